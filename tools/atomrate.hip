// atomrate.hip -- rate of returning device-scope atomic adds from every wave of a grid, as the queue appends make them
// (wavefront.h wave_reserve: one lane per wave adds to the queue's counter and waits for the old value).  Every wave
// makes `hops` dependent adds, either all to one word (a queue counter) or each wave to a word of its own, 128 bytes
// apart.  Reported per resident waves per SIMD: ns per add over the whole device (the serialisation on one word) and
// the latency one wave sees.  Usage: atomrate [hops]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

__global__ __launch_bounds__(256) void adds(unsigned *ctr, int stride_words, int hops, unsigned *out) {
  const unsigned wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  unsigned *c = ctr + (size_t)wave * stride_words;
  unsigned old = 0;
  if ((threadIdx.x & 63) == 0)
    for (int h = 0; h < hops; h++) old = atomicAdd(c + (old >> 31), 1u);  // (the address waits for the last add)
  if (old == 0xffffffffu) out[0] = old;
}

int main(int argc, char **argv) {
  const int hops = argc > 1 ? atoi(argv[1]) : 200;
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess) return 1;
  const size_t maxwaves = (size_t)ncu * 8 * 4;
  unsigned *ctr, *out;
  if (hipMalloc(&ctr, maxwaves * 128) != hipSuccess || hipMalloc(&out, 8) != hipSuccess) {
    printf("alloc failed\n");
    return 1;
  }
  (void)hipMemset(ctr, 0, maxwaves * 128);
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  for (int waves : {1, 2, 4, 8}) {
    const int blocks = ncu * waves;
    for (int stride : {0, 32}) {
      for (int rep = 0; rep < 2; rep++) {
        (void)hipEventRecord(a);
        adds<<<blocks, 256>>>(ctr, stride, hops, out);
        (void)hipEventRecord(b);
        (void)hipEventSynchronize(b);
        float ms;
        (void)hipEventElapsedTime(&ms, a, b);
        const double all = (double)blocks * 4 * hops;
        if (rep)
          printf("waves/SIMD %d %s: %8.3f ms  %7.2f ns per add (device)  %7.2f us per add (one wave)\n", waves,
                 stride ? "one word per wave" : "one word         ", ms, ms * 1e6 / all, ms * 1e3 / hops);
      }
    }
  }
  return 0;
}
