"""Build recipe for hidegs_amd/libhidegs.so (the C-ABI library of include/hidegs.h, hidegs_rows.h,
hidegs_resize.h, hidegs_clone.h, hidegs_topk.h, hidegs_nearest.h, hidegs_nearest_k.h, hidegs_nearest_within.h,
hidegs_nearest_lists.h, hidegs_voxel.h, hidegs_moments.h, hidegs_components.h, hidegs_neighbor_reduce.h and hidegs_neighbor_grad.h).

Built in-tree with hipcc for gfx950 so the .so travels to the GPU box with the
repository snapshot.  `python -m hidegs_amd.build` or `__graft_entry__.build()`.
Each source is compiled to its own object (in parallel) and linked once.  An object is
rebuilt when its source or a header is newer, or when its compile command (flags and
-D knobs) differs from the one recorded in its stamp file.

Test variants (VARIANTS) are the same library built with extra -D knobs into
hidegs_amd/variants/libhidegs_<tag>.so; the GPU tests load them to drive error paths
that the product build cannot reach (e.g. a tiny partition-queue job capacity).
"""
from __future__ import annotations

import concurrent.futures as cf
import glob
import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(HERE, "..", "include")
OBJDIR = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libhidegs.so")
VARIANT_DIR = os.path.join(HERE, "variants")
SOURCES = ["abi.cpp", "timing.cpp", "primitives.hip", "knn.hip", "adam.hip", "wire.hip", "rows.hip", "topk.hip",
           "nearest.hip", "voxel.hip", "moments.hip", "components.hip", "neighbor_reduce.hip", "neighbor_grad.hip"]
# every header: a change to any of them rebuilds every object
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(INCLUDE, "hidegs.h"),
                                                         os.path.join(INCLUDE, "hidegs_rows.h"),
                                                         os.path.join(INCLUDE, "hidegs_resize.h"),
                                                         os.path.join(INCLUDE, "hidegs_clone.h"),
                                                         os.path.join(INCLUDE, "hidegs_topk.h"),
                                                         os.path.join(INCLUDE, "hidegs_nearest.h"),
                                                         os.path.join(INCLUDE, "hidegs_nearest_k.h"),
                                                         os.path.join(INCLUDE, "hidegs_nearest_within.h"),
                                                         os.path.join(INCLUDE, "hidegs_nearest_lists.h"),
                                                         os.path.join(INCLUDE, "hidegs_voxel.h"),
                                                         os.path.join(INCLUDE, "hidegs_moments.h"),
                                                         os.path.join(INCLUDE, "hidegs_components.h"),
                                                         os.path.join(INCLUDE, "hidegs_neighbor_reduce.h"),
                                                         os.path.join(INCLUDE, "hidegs_neighbor_grad.h")]

# -ffp-contract=off: every fused multiply-add in the kernels is an explicit fmaf, so the
# oracle (oracle/knn_ref.c) can reproduce each rounding step bit for bit.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall",
         "-Wno-unused-function", "-I", INCLUDE]

# tag -> (extra defines, the sources they change); the other objects are shared with the product build
VARIANTS = {
    # partition-queue overflow -> error word; its starved workers give up after 2^16 polls (~0.2 s), not ~13 s
    "qcap": (["-DHIDEGS_JOB_CAP=64", "-DHIDEGS_MAX_POLLS=65536u"], ["primitives.hip"]),
    "gform": (["-DHIDEGS_QUEUE_MIN=8192"], ["primitives.hip"]),  # tiles of 2049..8192 pairs: one-workgroup global form
    "wscout": (["-DHIDEGS_WIDE_SCOUTS=1"], ["primitives.hip"]),  # hot tiles <= 12288 pairs as WIDE jobs (in place)
    "pcap": (["-DHIDEGS_PIECE_CAP=16"], ["primitives.hip"]),  # piece list full after 16: the rest as SMALL jobs
}


def hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP toolchain is required to build libhidegs.so")


def _command(src: str, obj: str, defines) -> list:
    lang = ["-x", "hip"] if src.endswith(".hip") else []
    return [hipcc(), *FLAGS, *defines, *lang, "-c", src, "-o", obj + ".tmp"]


def _stamp(cmd: list) -> str:
    # the command without the tool path and the output name: flags, knobs and the source
    return hashlib.sha256(" ".join(cmd[1:-2]).encode()).hexdigest()


def _stale(obj: str, src: str, stamp: str) -> bool:
    if not os.path.exists(obj) or not os.path.exists(obj + ".cmd"):
        return True
    with open(obj + ".cmd") as f:
        if f.read().strip() != stamp:
            return True
    t = os.path.getmtime(obj)
    return any(os.path.getmtime(p) > t for p in [src, *HEADERS])


def _compile(src: str, objdir: str, defines, verbose: bool) -> str:
    obj = os.path.join(objdir, os.path.basename(src) + ".o")
    cmd = _command(src, obj, defines)
    stamp = _stamp(cmd)
    if _stale(obj, src, stamp):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        os.replace(obj + ".tmp", obj)
        with open(obj + ".cmd", "w") as f:
            f.write(stamp + "\n")
    return obj


def _link(objs, lib: str, verbose: bool) -> str:
    if not os.path.exists(lib) or any(os.path.getmtime(o) > os.path.getmtime(lib) for o in objs):
        tmp = lib + ".tmp"
        cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", tmp]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        os.replace(tmp, lib)
    return lib


ABI_CLIENT_SRC = os.path.join(HERE, "..", "tests", "c_abi", "abi_client.cpp")
ABI_CLIENT = os.path.join(HERE, "..", "tests", "c_abi", "abi_client")


def build_abi_client(verbose: bool = False) -> str:
    """tests/c_abi/abi_client: a C++ program calling the ABI with no Python (test infrastructure, run on the
    GPU by tests/test_c_abi_gpu.py), linked against the in-tree library with an $ORIGIN-relative rpath."""
    deps = [ABI_CLIENT_SRC, LIB, os.path.join(INCLUDE, "hidegs.h")]
    if not os.path.exists(ABI_CLIENT) or any(os.path.getmtime(d) > os.path.getmtime(ABI_CLIENT) for d in deps):
        tmp = ABI_CLIENT + ".tmp"
        cmd = [hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", ABI_CLIENT_SRC,
               "-L" + HERE, "-lhidegs", "-Wl,-rpath,$ORIGIN/../../hidegs_amd", "-o", tmp]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        os.replace(tmp, ABI_CLIENT)
    return ABI_CLIENT


def variant_path(tag: str) -> str:
    return os.path.join(VARIANT_DIR, f"libhidegs_{tag}.so")


def _compile_all(sources, objdir: str, defines, verbose: bool) -> list:
    os.makedirs(objdir, exist_ok=True)
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(lambda s: _compile(os.path.join(CSRC, s), objdir, defines, verbose), sources))


def build_variant(tag: str, defines, changed=SOURCES, verbose: bool = False) -> str:
    """hidegs_amd/variants/libhidegs_<tag>.so: the library with `defines` on the `changed` sources; the
    other objects are the product build's (compiled here if stale)."""
    objs = dict(zip(changed, _compile_all(changed, os.path.join(VARIANT_DIR, "obj_" + tag), defines, verbose)))
    rest = [s for s in SOURCES if s not in objs]
    objs.update(zip(rest, _compile_all(rest, OBJDIR, [], verbose)))
    return _link([objs[s] for s in SOURCES], variant_path(tag), verbose)


def build(verbose: bool = False, variants: bool = True) -> str:
    _link(_compile_all(SOURCES, OBJDIR, [], verbose), LIB, verbose)
    if variants:
        with cf.ThreadPoolExecutor(max_workers=len(VARIANTS)) as ex:  # the product objects are fresh: no two compile one file
            list(ex.map(lambda tv: build_variant(tv[0], *tv[1], verbose=verbose), VARIANTS.items()))
        build_abi_client(verbose)
    return LIB


if __name__ == "__main__":
    print(build(verbose="-v" in sys.argv))
