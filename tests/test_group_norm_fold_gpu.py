"""The fixed-order folds of csrc/norm.hip at their edges.  gn_slab_kernel folds the PS pixel slots of a channel in batches of 16 LDS
reads (a partial last batch of PS % 16), gn_stats_kernel its PS * cpg items per group in batches of 8 per lane, gn_apply_kernel the rows of
`partials` in batches of 8 - in each case the adds of the plain loop in the plain loop's order.  The shapes below give the slab form

    (HW, C, groups)     cpg   gpb   PS    slots per thread
    (64, 1280, 32)      40    1     51    2 (the last slot ragged: 64 = 51 + 13)
    (256, 1280, 32)     40    1     51    6
    (256, 640, 32)      20    2     51    6
    (100, 320, 32)      10    4     51    2 (ragged)
    (64, 1280 + 1280, 32) 80  1     25    3 (two sources; cpg no power of two, 25 = 16 + 9)
    (200, 512, 32)      16    1     128   2 (eight whole batches, no partial one)
    (1024, 640, 32)     20    2     51    21 (the 24-pixel register class, a shape of the 512 x 512 pipeline)

and the two-launch form: (4096, 320, 32) at N = 2 - 64 rows of partials per sample, 16 per thread of the apply pass, 60 LDS items per group
of the statistics pass (one partial batch per lane) - and (1600, 72, 2) - 28 pixel slots x 36 channels = 1008 items per group, 126 per lane:
fifteen whole batches and a partial one.

Per case: the route the table declares, every operand between NaN guards, the same launch twice bit for bit, the N-sample launch bit for bit
its N one-sample launches (the promise of gn_slab_gpb's comment), and the fp64 bars of tests/test_norm_gpu.py (its helpers, unchanged)."""
import pytest
import torch

from tests import numerics as nm
from tests import test_numerics_gpu as T
from tests import test_norm_gpu as NG
from tests.test_numerics_gpu import judge, done

pytestmark = pytest.mark.gpu

#        HW    C1    C2    groups N  class        route fields
CASES = [(64, 1280, 0, 32, 3, "slab-8", dict(gpb=1, slots=51)),
         (256, 1280, 0, 32, 3, "slab-8", dict(gpb=1, slots=51)),
         (256, 640, 0, 32, 3, "slab-8", dict(gpb=2, slots=51)),
         (100, 320, 0, 32, 3, "slab-8", dict(gpb=4, slots=51)),
         (64, 1280, 1280, 32, 3, "slab-8", dict(gpb=1, slots=25)),
         (200, 512, 0, 32, 3, "slab-8", dict(gpb=1, slots=128)),
         (1024, 640, 0, 32, 3, "slab-24", dict(gpb=2, slots=51)),
         (4096, 320, 0, 32, 2, "two-fixed", dict(nchunk=64, ppb=64, ps=6)),
         (1600, 72, 0, 2, 2, "two-fixed", dict(nchunk=64, ppb=25, ps=28))]


def case_id(c):
    return f"HW{c[0]}-C{c[1]}+{c[2]}-G{c[3]}-N{c[4]}"


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T._name)
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_group_norm_folds_keep_order_and_bits(case, silu, dtype):
    HW, C1, C2, groups, N, cls, fields = case
    name = f"norm fold {case_id(case)} silu{int(silu)} {T._name(dtype)}"
    c = nm.norm_case(HW, C1, C2, groups, N, "ratio_30", dtype, silu=silu, seed=HW + C1 + 7 * N)
    route = NG.gn_route_of(N, HW, C1, C2, groups)
    assert route == nm.gn_route(N, HW, C1 + C2, groups), (route, nm.gn_route(N, HW, C1 + C2, groups))
    assert NG.route_class(route) == cls and all(route[k] == v for k, v in fields.items()), route
    y, _, problems = NG.gn_launch(c, dtype)
    y2, _, p2 = NG.gn_launch(c, dtype)
    fails = [f"{name}: {p}" for p in problems + p2]
    if not torch.equal(y, y2):
        fails.append(f"{name}: the same launch twice differs in {nm.differs(y, y2, count=True)} elements")
    for n in range(N):
        y1, _, p1 = NG.gn_launch(c, dtype, n, n + 1)
        fails += [f"{name} sample {n} alone: {p}" for p in p1]
        if not torch.equal(y1[0], y[n]):
            fails.append(f"{name}: sample {n} launched alone differs from the N = {N} launch in {nm.differs(y1[0], y[n], count=True)} elements")
    ref = nm.gn_ref64(c)
    e_alg, e_ref = nm.row_err(nm.gn_base_alg(c, geom=route), ref), nm.row_err(nm.gn_base_ref(c), ref)
    print(f"{name}: row_err kernel {nm.row_err(y, ref):.3e}, base_alg {e_alg:.3e}, base_ref {e_ref:.3e}")
    judge(fails, name, y, ref, e_alg, e_ref, dtype)
    done(fails)
