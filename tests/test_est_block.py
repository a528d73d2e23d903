"""Host check of the estimator block's single description (artis_amd/csrc/engine/est_block.h): the sections are
contiguous and in the ABI's order, EstLayout's named offsets are theirs, pack puts every field into its section and
nowhere else, unpack(pack(x)) is the identity, missing arrays pack as zeros and are skipped (within bounds) by unpack,
and average_scalars changes exactly the eight time-step scalars.  tests/est_block_check.cpp includes that header alone
and is built with hipcc for the host (no GPU needed); it runs once plain and once as a stand-alone executable under
the host address / undefined sanitizers."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def _build(exe, extra):
    return subprocess.run([HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", *extra, "-I", os.path.join(REPO, "include"),
                           "-I", os.path.join(REPO, "artis_amd", "csrc", "engine"), "-x", "c++",
                           os.path.join(REPO, "tests", "est_block_check.cpp"), "-o", str(exe)],
                          capture_output=True, text=True, timeout=300)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("sanitized", [False, True])
def test_est_block(tmp_path, sanitized):
    exe = tmp_path / "est_block_check"
    b = _build(exe, SANITIZE if sanitized else [])
    if sanitized and b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitizer" in b.stderr):
        pytest.skip("the host sanitizer runtime is not installed")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad 0" in r.stdout
