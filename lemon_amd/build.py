"""Builds liblemon_hip.so (the C-ABI HIP library) in-tree for gfx950.

hipcc cross-compiles without a GPU, so this also runs in the CPU-only build container.  Each
translation unit is compiled to an object under lemon_amd/csrc/_obj/ (only when it or a header
changed, several at a time) and the objects are linked into the shared library.
"""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
SO = os.path.join(HERE, "liblemon_hip.so")
SOURCES = ["api.hip", "rowwise.hip", "knn_f32.hip", "knn_bf16.hip", "attention.hip", "attention_hd.hip", "attention_varlen.hip", "linear.hip", "preprocess.hip",
           "gridf1.hip", "ksweep.hip", "dedup.hip", "encoder.hip", "gemm_f16x3.hip", "kmeans.hip", "jpeg.hip", "jpeg_entropy.hip", "jpeg_prog.hip", "tokenize.hip", "hparam_search.hip", "lbfgs_polish.hip", "discrepancy_ks.hip", "metric_sweep.hip", "eval_metrics.hip", "png.hip", "png_inflate.hip"]
HEADERS = ["common.hpp", "knn_common.hpp", "split3.hpp", "attention_hd64.hpp", "attention_plan.hpp", "scan_plan.hpp", "knn_wide.hpp", "knn_bf16_plan.hpp", "gemm_f16x3_plan.hpp", "jpeg_core.hpp", "jpeg_entropy.hpp", "jpeg_par.hpp", "jpeg_abi.hpp",
           "jpeg_prog.hpp", "jpeg_prog_par.hpp", "tokenize_core.hpp", "gridf1_brent.hpp", "hparam_search_core.hpp", "lbfgs_core.hpp", "chain_dist.hpp", "discrepancy_core.hpp", "l2_from_ip_core.hpp", "index_ws.hpp", "eval_metrics_core.hpp", "png_core.hpp", "png_abi.hpp", "png_inflate_core.hpp", os.path.join("..", "..", "include", "lemon_hip.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]
# the JPEG host pass and the PNG chunk parser alone, built with the host compiler: no HIP runtime, loaded by the decode workers
# (decode_worker.py)
JPEG_HOST_SO = os.path.join(HERE, "liblemon_jpeg_host.so")
JPEG_HOST_SOURCE = "jpeg_host.cpp"
JPEG_HOST_HEADERS = ["jpeg_core.hpp", "jpeg_entropy.hpp", "jpeg_par.hpp", "jpeg_abi.hpp", "jpeg_prog.hpp", "jpeg_prog_par.hpp", "png_core.hpp", "png_abi.hpp", "png_inflate_core.hpp",
                     os.path.join("..", "..", "include", "lemon_hip.h")]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: liblemon_hip.so cannot be built")


def _sources():
    return [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(p) > t for p in deps)


def _host_cxx():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    raise RuntimeError("no host C++ compiler found: liblemon_jpeg_host.so cannot be built")


def _jpeg_host_deps():
    return [os.path.join(CSRC, s) for s in [JPEG_HOST_SOURCE] + JPEG_HOST_HEADERS]


def build_jpeg_host(force=False, verbose=False):
    if not force and not _stale(JPEG_HOST_SO, _jpeg_host_deps()):
        return JPEG_HOST_SO
    cmd = [_host_cxx(), "-O3", "-std=c++17", "-fPIC", "-shared", "-o", JPEG_HOST_SO, os.path.join(CSRC, JPEG_HOST_SOURCE)]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return JPEG_HOST_SO


def needs_build():
    deps = [os.path.join(CSRC, s) for s in _sources() + HEADERS]
    return _stale(SO, deps) or _stale(JPEG_HOST_SO, _jpeg_host_deps())


def build_hip(force=False, verbose=False, jobs=None):
    if not force and not needs_build():
        return SO
    build_jpeg_host(force, verbose)
    if not force and not needs_build():
        return SO
    hipcc = _hipcc()
    os.makedirs(OBJ, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    todo, objs = [], []
    for s in _sources():
        src, obj = os.path.join(CSRC, s), os.path.join(OBJ, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, [src] + hdrs):
            todo.append([hipcc] + FLAGS + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    if todo:
        with ThreadPoolExecutor(max_workers=jobs or min(4, len(todo))) as pool:
            list(pool.map(run, todo))
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO] + objs + ["-lhipblaslt"])
    return SO


if __name__ == "__main__":
    import sys
    print(build_hip(force="--force" in sys.argv, verbose=True))
