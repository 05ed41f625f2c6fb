"""Build an experimental variant of libhidegs.so with extra compile definitions.

usage: python tools/build_variant.py TAG -DNAME=VALUE ...   ->  hidegs_amd/variants/libhidegs_TAG.so
Run a tool against it with HIDEGS_LIB=hidegs_amd/variants/libhidegs_TAG.so (hidegs_amd/_lib.py).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hidegs_amd import build  # noqa: E402

if __name__ == "__main__":
    print(build.build_variant(sys.argv[1], sys.argv[2:], verbose=True))
