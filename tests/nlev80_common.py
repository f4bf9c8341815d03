"""What the 80-level tests share: the 80-level grid (tests/golden/vcoord/12k_top-80{m,i}.ascii, made by tests/vcoord_levels.py) and
tests/remap_ld.py's input families on it.  remap_ld.hvcoord knows the 72- and the 64-level grid; importing this module teaches it the
80-level one, so that remap_ld.grids / inputs / uniform_inputs (written for any level count) build their columns on it."""
import numpy as np

import remap_ld as rl
import vcoord_levels as vl
from transport_se_amd.hybvcoord import HvCoord

NLEV = 80
# tracer counts of the 80-level remap tests (16 tracer slots per block): 1, 2 and 3 leftover tracers as segment tasks only (1, 2, 3),
# no segment task (7: one partly idle round), a whole round and 3 segment tracers (19)
REMAP_QSIZES = (1, 2, 3, 7, 19)


def hv80():
    return HvCoord(*vl.paths(NLEV))


_hvcoord = rl.hvcoord


def _hvcoord_80(nlev):
    return hv80() if nlev == NLEV else _hvcoord(nlev)


rl.hvcoord = _hvcoord_80   # (a module body runs once per process)


def kid_offsets(dp1, dp2):
    """kid(k) - k of every column [nlev][E][16] (remap_ld.grid_fp64: the reference's bracket search on the fp64 serial sums)"""
    E, nlev = dp1.shape[:2]
    _, _, _, kid = rl.grid_fp64(np.moveaxis(dp1.reshape(E, nlev, 16), 1, 0).reshape(nlev, -1),
                                np.moveaxis(dp2.reshape(E, nlev, 16), 1, 0).reshape(nlev, -1))
    return (kid - np.arange(1, nlev + 1)[:, None]).reshape(nlev, E, 16)
