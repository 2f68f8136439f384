"""In-tree build of the HIP extension (libsdbv.so) for gfx950.

The .so is built in-tree so it travels with the repo snapshot to GPU boxes
(JIT caches under ~/.cache do not). hipcc cross-compiles on CPU-only hosts.
"""
import os
import subprocess

_DIR = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_DIR, "libsdbv.so")
SRC = os.path.join(_DIR, "csrc", "sdbv.hip")

# -ffp-contract=off is LOAD-BEARING: hipcc contracts a*b+c into v_fma_f32
# even through __fmul_rn/__fadd_rn (verified on ROCm 7.2/gfx950); the
# reference (rustc/LLVM) never contracts, and the parity contract requires
# the exact mul-then-add rounding per element. The scan is HBM-bound, so the
# extra VALU ops cost nothing.
CMD = [
    "hipcc",
    "--offload-arch=gfx950",
    "-O3",
    "-ffp-contract=off",
    # The l2 prefilter's proof (pf_l2_finish) needs the device's f32 sqrt
    # correctly rounded, as the host's is. It is the compiler's default for
    # HIP; spelled out because a bound rests on it.
    "-fhip-fp32-correctly-rounded-divide-sqrt",
    # AVX2 for the HOST build path (graph construction distance chains).
    # Bit-exactness holds: the restated unrolled-8 chain keeps 8 independent
    # sequential partials, which vectorize to one 8-lane register without
    # reassociation, and -ffp-contract=off still blocks mul+add fusion.
    "-Xarch_host",
    "-mavx2",
    "-std=c++17",
    "-fPIC",
    "-shared",
    SRC,
    "-L/opt/rocm/lib",
    "-lrocblas",
    "-o",
    SO_PATH,
]


def build(force=False):
    if (not force and os.path.exists(SO_PATH)
            and os.path.getmtime(SO_PATH) >= os.path.getmtime(SRC)):
        return SO_PATH
    subprocess.run(CMD, check=True)
    return SO_PATH


if __name__ == "__main__":
    print(build(force=True))
