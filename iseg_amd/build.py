"""Build libiseg_hip.so (gfx950) in-tree with hipcc.  `python -m iseg_amd.build` or build() from __graft_entry__."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libiseg_hip.so")
SOURCES = ["api.hip", "gemm.hip", "gemm_nn.hip", "gemm_nt.hip", "gemm_tn.hip", "norm.hip", "dwconv.hip", "dwconv_mfma.hip", "dwconv_wgrad_mfma.hip", "dwconv_strided.hip", "elementwise.hip", "resize.hip", "loss.hip", "confusion.hip", "ohem.hip", "mask_loss.hip", "sod_metrics.hip", "sod_fmv2.hip", "ccl.hip", "optim.hip", "misc.hip", "attention.hip", "dcnv3.hip", "defattn.hip", "winattn.hip", "flashattn.hip", "selfattn.hip", "mlp_fused.hip", "mlp_wgrad.hip", "mlp_bwd_onepass.hip", "conv_igemm.hip", "conv_patchify.hip", "augment.hip", "projective.hip", "grn.hip", "eva.hip", "comm.hip", "mbconv.hip", "sepconv.hip", "jpu.hip", "resblock.hip", "gemma.hip", "gemma_decode.hip", "decode_commit.hip", "token_sample.hip", "beam_search.hip", "contrastive.hip", "lm_head_ce.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
         "-Wno-unused-result"] + [f"-D{d}" for d in os.environ.get("ISEG_BUILD_DEFINES", "").split() if d]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    os.makedirs(LIBDIR, exist_ok=True)
    hipcc = _hipcc()
    headers = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join(ROOT, "include", "iseg_hip.h")]
    objs, jobs = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(LIBDIR, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, [src] + headers):
            jobs.append([hipcc] + FLAGS + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    if jobs or not os.path.exists(LIB):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
