// estimators_host.h -- the readout side of the estimators: artis_gpu_estimators_zero / _download, the packed device
// block (artis_gpu_estimator_block_doubles / _to_device / _from_device) and its RCCL all-reduce (artis_gpu_comm_*,
// artis_gpu_estimators_allreduce), with their two small kernels.  The block's sections, their lengths and the member
// of artis_estimators each carries come from the layout the engine computed at init (G.est, est_block.h); nothing
// here knows an offset.  Included once by engine.hip after engine_state.h (G, HIPCHK, dmalloc).
#pragma once

// the block's tail on the device: the line counters and DevEst::counters as doubles (dir 0) and back (dir 1)
__global__ void k_pack_counts(const int32_t *ecounter, const int32_t *acounter, const unsigned long long *counters,
                              double *dst, int nlines, int dir) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = 2 * (int64_t)nlines + ARTIS_COUNTER_COUNT + 1;
  if (i >= n) return;
  if (dir == 0) {
    if (i < nlines)
      dst[i] = ecounter[i];
    else if (i < 2 * nlines)
      dst[i] = acounter[i - nlines];
    else
      dst[i] = (double)counters[i - 2 * nlines];
  } else {
    if (i < nlines)
      const_cast<int32_t *>(ecounter)[i] = (int32_t)llrint(dst[i]);
    else if (i < 2 * nlines)
      const_cast<int32_t *>(acounter)[i - nlines] = (int32_t)llrint(dst[i]);
    else
      const_cast<unsigned long long *>(counters)[i - 2 * nlines] = (unsigned long long)llrint(dst[i]);
  }
}

#define NCCLCHK(x)                                                                            \
  do {                                                                                        \
    ncclResult_t r_ = (x);                                                                    \
    if (r_ != ncclSuccess) {                                                                  \
      G.last_error = std::string(#x) + ": " + ncclGetErrorString(r_);                         \
      return ARTIS_ERR_HIP;                                                                   \
    }                                                                                         \
  } while (0)

namespace {

int pack_counts(double *block, int dir) {
  const DevEst &E = G.K.E;
  k_pack_counts<<<(unsigned)((G.est.block.tail() + 255) / 256), 256, 0, G.stream>>>(
      E.ecounter, E.acounter, E.counters, block + G.est.n_doubles, G.nlines, dir);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(G.stream));
  return 0;
}

}  // namespace

extern "C" {

int artis_gpu_estimators_zero(void) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  const DevEst &E = G.K.E;
  const EstSection *S = G.est.block.s;
  HIPCHK(hipMemsetAsync(G.d_estblock, 0, (size_t)G.est.n_doubles * sizeof(double), G.stream));
  HIPCHK(hipMemsetAsync(E.ecounter, 0, (size_t)S[ES_ECOUNTER].n * sizeof(int32_t), G.stream));
  HIPCHK(hipMemsetAsync(E.acounter, 0, (size_t)S[ES_ACOUNTER].n * sizeof(int32_t), G.stream));
  HIPCHK(hipMemsetAsync(E.counters, 0, (size_t)(S[ES_COUNTERS].n + S[ES_NESC].n) * sizeof(unsigned long long),
                        G.stream));
  return 0;
}

// ADD the device's sums into *est: the double block as it is, behind it the integer counters as the doubles
// k_pack_counts makes of them
int artis_gpu_estimators_download(artis_estimators *est) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  if (!est) return ARTIS_ERR_BAD_ARGUMENT;
  HIPCHK(hipStreamSynchronize(G.stream));
  const EstBlock &B = G.est.block;
  const DevEst &E = G.K.E;
  std::vector<double> blk(B.len, 0.);
  HIPCHK(hipMemcpy(blk.data(), G.d_estblock, (size_t)B.n_device * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<int32_t> lc(G.nlines);
  for (int k : {ES_ECOUNTER, ES_ACOUNTER}) {
    HIPCHK(hipMemcpy(lc.data(), k == ES_ECOUNTER ? E.ecounter : E.acounter, lc.size() * sizeof(int32_t),
                     hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < B.s[k].n; j++) blk[B.s[k].off + j] = lc[j];
  }
  std::vector<unsigned long long> ctr(B.s[ES_COUNTERS].n + B.s[ES_NESC].n);
  HIPCHK(hipMemcpy(ctr.data(), E.counters, ctr.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  for (size_t j = 0; j < ctr.size(); j++) blk[B.s[ES_COUNTERS].off + j] = (double)ctr[j];
  est_block_unpack(B, blk.data(), est, true);
  return 0;
}

size_t artis_gpu_estimator_block_doubles(void) { return G.initialised ? (size_t)G.est.block.len : 0; }

int artis_gpu_estimator_block_to_device(void *dst) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  HIPCHK(hipMemcpyAsync(dst, G.d_estblock, (size_t)G.est.n_doubles * sizeof(double), hipMemcpyDeviceToDevice, G.stream));
  return pack_counts((double *)dst, 0);
}

int artis_gpu_estimator_block_from_device(const void *src) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  HIPCHK(hipMemcpyAsync(G.d_estblock, src, (size_t)G.est.n_doubles * sizeof(double), hipMemcpyDeviceToDevice, G.stream));
  return pack_counts(const_cast<double *>((const double *)src), 1);
}

int artis_gpu_comm_unique_id(void *id) {
  if (!id) return ARTIS_ERR_BAD_ARGUMENT;
  static_assert(sizeof(ncclUniqueId) == ARTIS_COMM_ID_BYTES, "RCCL unique id size");
  ncclUniqueId uid;
  NCCLCHK(ncclGetUniqueId(&uid));
  memcpy(id, &uid, sizeof uid);
  return 0;
}

int artis_gpu_comm_init(int rank, int nranks, const void *id) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  if (!id || nranks <= 0 || rank < 0 || rank >= nranks) return ARTIS_ERR_BAD_ARGUMENT;
  artis_gpu_comm_finalize();
  HIPCHK(hipSetDevice(G.device));
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof uid);
  NCCLCHK(ncclCommInitRank(&G.comm, nranks, uid, rank));
  G.comm_ranks = nranks;
  if (!G.d_redblock) HIPCHK(dmalloc((void **)&G.d_redblock, artis_gpu_estimator_block_doubles() * sizeof(double)));
  return 0;
}

// mpi_reduce_estimators divides the eight time_step scalars by nprocs after the sum (sn3d.cc:370-377): every rank
// carries a full-energy ensemble.  The arrays stay sums (update_grid divides them by nprocs, update_grid.cc:1041).
__global__ void k_average_timestep_scalars(double *sc, int nranks) {
  if (threadIdx.x < 8) sc[threadIdx.x] /= nranks;
}
static_assert(EST_AVERAGED == 8, "k_average_timestep_scalars averages the first eight scalars");

int artis_gpu_estimators_allreduce(void) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  if (!G.comm || !G.d_redblock) {
    G.last_error = "artis_gpu_comm_init must precede artis_gpu_estimators_allreduce";
    return ARTIS_ERR_BAD_ARGUMENT;
  }
  if (int rc = artis_gpu_estimator_block_to_device(G.d_redblock)) return rc;
  NCCLCHK(ncclAllReduce(G.d_redblock, G.d_redblock, artis_gpu_estimator_block_doubles(), ncclFloat64, ncclSum, G.comm,
                        G.stream));
  k_average_timestep_scalars<<<1, 64, 0, G.stream>>>(G.d_redblock + G.est.scalars, G.comm_ranks);
  HIPCHK(hipGetLastError());
  return artis_gpu_estimator_block_from_device(G.d_redblock);
}

void artis_gpu_comm_finalize(void) {
  if (G.comm) {
    (void)hipStreamSynchronize(G.stream);
    (void)ncclCommDestroy(G.comm);
  }
  G.comm = nullptr;
  G.comm_ranks = 0;
}

}  // extern "C"
