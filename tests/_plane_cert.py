"""The stand-alone host build of octreelib_amd/csrc/plane_cert.h (tests/host/plane_cert_host.cpp) and, re-exported, the
NumPy model of the certified exit (tools/plane_cert_model.py): shared by tests/test_cpu_plane_cert.py and
tests/test_gpu_ransac_cert_exit.py."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from plane_cert_model import (block_constants, certified, cross_floor, margin_all, no_plane_holds_all,  # noqa: E402,F401
                              no_plane_holds_others, scatter, vouched)


# ---- the stand-alone host build of plane_cert.h ---------------------------------------------------------------------------
def build_host_program(directory):
    """tests/host/plane_cert_host.cpp compiled for the CPU alone with AddressSanitizer and UBSan; returns the program."""
    exe = os.path.join(str(directory), "plane_cert_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "octreelib_amd", "csrc"), os.path.join(ROOT, "tests", "host", "plane_cert_host.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def run_host_program(exe, directory, blocks, ts):
    """(len(blocks), 2) bool: the program's two verdicts per block."""
    fin, fout = os.path.join(str(directory), "cert_in.bin"), os.path.join(str(directory), "cert_out.bin")
    with open(fin, "wb") as f:
        f.write(np.int64(len(blocks)).tobytes())
        for p, t in zip(blocks, ts):
            f.write(np.int64(len(p)).tobytes())
            f.write(np.float64(t).tobytes())
            f.write(np.ascontiguousarray(p, dtype=np.float64).tobytes())
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    v = np.fromfile(fout, dtype=np.uint8)
    assert len(v) == 2 * len(blocks)
    return v.reshape(-1, 2).astype(bool)
