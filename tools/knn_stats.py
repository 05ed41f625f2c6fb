"""distCUDA2's phase-1 search statistics for a few point sets: per wave the candidate leaves and points
evaluated, the waves that bailed out to phase 2, and the wave-duration profile.  The library prints them
(stderr) from its statistics build only (hidegs_amd/csrc/knn_stats.h):

    python tools/build_variant.py kstats -DHIDEGS_KNN_STATS=1
    python tools/knn_stats.py [SET ...]      (default: every set)

For times use tools/knn_time.py on the product build: the statistics build synchronises in every call.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "hidegs_amd", "variants", "libhidegs_kstats.so")
if not os.path.exists(LIB):
    sys.exit(f"{LIB} is missing: build it with `python tools/build_variant.py kstats -DHIDEGS_KNN_STATS=1`")
os.environ["HIDEGS_LIB"] = LIB  # read when hidegs_amd._lib is imported
import numpy as np  # noqa: E402
import torch  # noqa: E402

import simple_knn  # noqa: E402
from hidegs_amd import synthetic  # noqa: E402
from knn_stress import core_shell  # noqa: E402

SETS = {
    "frustum2M": lambda: synthetic.frustum_points(2_000_000),
    "uniform2M": lambda: torch.rand(2_000_000, 3),
    "plane2M": lambda: torch.cat([torch.rand(2_000_000, 2), torch.zeros(2_000_000, 1)], 1),
    # the input of tests/test_knn_gpu.py::test_bail_out_wave_every_point
    "core_shell40k": lambda: torch.from_numpy(core_shell(np.random.default_rng(7), 28_000, 12_000)),
    # the input of tests/test_knn_every_point_gpu.py::test_core_shell_700k_every_point
    "core_shell700k": lambda: torch.from_numpy(core_shell(np.random.default_rng(7), 490_000, 210_000)),
}
for name in sys.argv[1:] or SETS:
    print(name, flush=True)
    simple_knn._C.distCUDA2(SETS[name]().cuda())
    torch.cuda.synchronize()
