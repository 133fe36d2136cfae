"""csrc/norm.hip on every route: gn_stats_kernel + gn_apply_kernel (both streaming loops), gn_slab_kernel in its three register classes and
layer_norm_kernel in its five, judged per row against fp64 (tests/numerics.py, the norm section; method: tests/NUMERICS.md):
row_err(kernel) <= MARGIN x base_alg - the algorithm in the chunk geometry of the form that RUNS -, <= MARGIN x base_ref (every row is in
the required tier: |mean| / std <= 30), finite wherever the rounded fp64 result is.

Every operand of every launch - x, x2, out, partials, gamma, beta - is a slice from the middle of a buffer with NaN guards on each side
(payload NaNs in the fp16 / bf16 inputs; out and partials pre-filled with NaN).  Afterwards the guards are bit for bit what they were, the out
slice holds no NaN and in `partials` exactly the route's nchunk rows per sample are finite (a slab launch leaves all of it NaN).  Every launch
runs twice and must repeat bit for bit; every row runs at N = 3 and must equal three N = 1 launches bit for bit (gn_slab_gpb: the route never
depends on N), a grouped launch its per-set launches.  The route is asserted at run time from es_group_norm_route / es_layer_norm_route - the
launcher's own code - against the one the table declares, and at import the table is placed by nm.gn_route, the CPU mirror of that rule.

LN_TABLE is no cross product either: every C runs with 13 rows (three whole 4-row workgroups and one row of a fourth) and with ONE of
M = 1, 3, 4, 5 in rotation, so that every VPL instantiation meets 13 and at least one short launch; a row's result does not depend on M
(each row is also launched alone and must give the same bits).

GN_TABLE is not a cross product: every input kind (nm.NORM_KINDS) meets every route class at least once, which `coverage()` asserts at import."""
import ctypes
import time

import pytest
import torch
import torch.nn.functional as F

from tests import numerics as nm
from tests import test_numerics_gpu as T
from tests.test_numerics_gpu import judge, done

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096                    # elements of NaN in front of and behind x, x2 and out
PGUARD = 256                    # ... gamma and beta (fp32)
RECORD = []                     # one dict per judged launch (python -m tests.numerics --report --only norm writes them to NUMERICS.md)
N_ROW = 3
SPLIT = (104, 216)              # C = 320 as two sources: workgroup 3 of the slab (channels 120 .. 159 at gpb 4) and group 10 (100 .. 109) straddle them

GN_CLASSES = ("slab-8", "slab-16", "slab-24", "two-fixed", "two-4lane", "two-general")


def route_class(r):
    if r["form"] == nm.GN_FORM_SLAB:
        return f"slab-{r['cpt']}"
    return "two-general" if r["general"] else "two-4lane" if r["lanes"] == 4 else "two-fixed"


def G(HW, C1, C2, groups, cls, kinds, **route):
    """one geometry and the kinds it meets; `route`: the route fields the issue names for it (asserted against the mirror and the library)"""
    return [dict(HW=HW, C1=C1, C2=C2, groups=groups, cls=cls, kind=k, route=route) for k in kinds]


GN_TABLE = sum([
    # ---- one launch (slab) ----
    G(1, 8, 0, 1, "slab-8", ("ratio_0", "zero")),
    G(1, 320, 0, 32, "slab-8", ("ratio_0",), gpb=4),
    G(15, 640, 0, 32, "slab-8", ("ratio_0", "zero"), gpb=2),
    G(9, 1280, 0, 32, "slab-8", ("constant", "dominant"), gpb=1, slots=51),            # 51 slots x 5 chunks: 255 active threads
    G(64, 2560, 0, 32, "slab-8", ("ratio_30",)),
    G(256, 24, 0, 1, "slab-8", ("dominant",)),
    G(600, 128, 0, 64, "slab-8", ("ratio_30", "constant"), gpb=4),                      # cpg 2
    G(24, 2048, 0, 1, "slab-24", ("ratio_30", "zero"), gpb=1, slots=1),                 # W8 = 256: one pixel slot, 24 pixels per thread
    G(408, 320, 0, 32, "slab-8", ("ratio_30",), gpb=4), G(408, *SPLIT, 32, "slab-8", ("ratio_0",), gpb=4),
    G(409, 320, 0, 32, "slab-16", ("ratio_0", "constant"), gpb=4), G(409, *SPLIT, 32, "slab-16", ("ratio_30", "zero"), gpb=4),
    G(816, 320, 0, 32, "slab-16", ("dominant", "ratio_30"), gpb=4), G(816, *SPLIT, 32, "slab-16", ("ratio_0",), gpb=4),
    G(817, 320, 0, 32, "slab-24", ("ratio_0", "zero"), gpb=4), G(817, *SPLIT, 32, "slab-24", ("ratio_30",), gpb=4),
    G(1224, 320, 0, 32, "slab-24", ("dominant", "constant"), gpb=4), G(1224, *SPLIT, 32, "slab-24", ("ratio_0",), gpb=4),
    # ---- two launches ----
    G(1225, 320, 0, 32, "two-fixed", ("ratio_0", "ratio_30", "zero"), nchunk=62, ppb=20),       # 35 x 35: 65 chunks before the chunk rule was rounded up
    G(1296, 320, 0, 32, "two-fixed", ("dominant", "constant"), nchunk=62, ppb=21),              # 36 x 36: 65 before
    G(25, 2048, 0, 1, "two-fixed", ("ratio_30", "zero"), ps=1),
    G(1, 8, 0, 8, "two-fixed", ("constant", "zero"), ps=256, ppb=16),                           # more pixel slots than pixels
    G(7, 8, 16, 8, "two-fixed", ("ratio_0",)), G(17, 8, 16, 8, "two-fixed", ("ratio_30", "zero")),      # cpg 3: group 2 (channels 6 .. 8) straddles the sources
    G(100, 8, 16, 8, "two-fixed", ("dominant", "constant")),
    G(1087, 8, 16, 8, "two-fixed", ("ratio_0", "ratio_30"), nchunk=64, ppb=17),                 # 68 chunks before
    G(4225, 64, 0, 64, "two-4lane", ("ratio_0", "ratio_30", "constant"), nchunk=64, ppb=67),    # 65 x 65: 65 before
    G(50, 120, 0, 40, "two-4lane", ("dominant", "zero", "ratio_0")),
    G(300, 1040, 0, 8, "two-general", ("ratio_0", "dominant"), ps=1),
    G(5, 2056, 0, 1, "two-general", ("ratio_30", "zero")),
    G(49, 8000, 0, 32, "two-general", ("constant", "ratio_0"), lds=(2 * 8000 + 64 + 256) * 4),  # 65 280 bytes of LDS: 256 under the limit
], [])
for _i, _row in enumerate(GN_TABLE):
    _row["silu"] = _i % 2 == 0
    _row["seed"] = 11 * _i + 5

GN_GROUPED = [(409, *SPLIT, 32, "slab-16"), (1087, 8, 16, 8, "two-fixed")]
GN_STATS_ONLY = [(1225, 320, 32), (50, 120, 40), (300, 1040, 8)]

LN_CS = (8, 504, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 4096)
LN_VPL = {8: 1, 504: 1, 512: 1, 520: 2, 1024: 2, 1032: 3, 1536: 3, 1544: 4, 2048: 4, 2056: 8, 4096: 8}
LN_TABLE = [dict(M=13, C=C, ratio=(0, 30)[i % 2]) for i, C in enumerate(LN_CS)] + \
           [dict(M=(1, 3, 4, 5)[i % 4], C=C, ratio=(30, 0)[i % 2]) for i, C in enumerate(LN_CS)] + \
           [dict(M=5, C=1024, ratio=300), dict(M=4, C=2056, ratio=300)]     # where a one-pass variance would show (fp16; test_numerics_cpu.py)


def gn_id(row):
    return f"HW{row['HW']}-C{row['C1']}+{row['C2']}-G{row['groups']}-{row['kind']}-silu{int(row['silu'])}"


def ln_id(row):
    return f"M{row['M']}-C{row['C']}-ratio{row['ratio']}"


def coverage():
    """route class x input kind -> number of rows; returns (text, the unmet cells)"""
    lines, missing = [], []
    for cls in GN_CLASSES:
        cells = {k: sum(r["cls"] == cls and r["kind"] == k for r in GN_TABLE) for k in nm.NORM_KINDS}
        missing += [(cls, k) for k, v in cells.items() if not v]
        lines.append(f"{cls:<12} " + "  ".join(f"{k}: {v}" for k, v in cells.items()))
    two = [r for r in GN_TABLE if r["cls"].startswith("two")]
    for silu in (True, False):
        if not any(r["silu"] == silu for r in two):
            missing.append(("two launches", f"silu {silu}"))
    for vpl in (1, 2, 3, 4, 8):
        ms = sorted({r["M"] for r in LN_TABLE if LN_VPL[r["C"]] == vpl})
        lines.append(f"LayerNorm VPL {vpl}: M {ms}")
        if 13 not in ms or len(ms) < 2:
            missing.append(("VPL", vpl))
    return "\n".join(lines), missing


for _row in GN_TABLE:
    _r = nm.gn_route(N_ROW, _row["HW"], _row["C1"] + _row["C2"], _row["groups"])
    assert route_class(_r) == _row["cls"] and all(_r[k] == v for k, v in _row["route"].items()), (gn_id(_row), _r)
    assert _r["lds"] <= nm.GN_LDS_LIMIT and N_ROW * _row["HW"] * (_row["C1"] + _row["C2"]) <= 3 * 420000
    assert _r == nm.gn_route(1, _row["HW"], _row["C1"] + _row["C2"], _row["groups"]), "at these sizes the route must not depend on N"
_matrix, _missing = coverage()
assert not _missing, f"test_norm_gpu.GN_TABLE leaves unmet: {_missing}\n{_matrix}"
assert len({gn_id(r) for r in GN_TABLE}) == len(GN_TABLE) and len({ln_id(r) for r in LN_TABLE}) == len(LN_TABLE)
assert {r["M"] for r in LN_TABLE} == {1, 3, 4, 5, 13} and {r["C"] for r in LN_TABLE} == set(LN_CS)


# ----------------------------------------------------------------------------------------------------------------
# guarded operands
# ----------------------------------------------------------------------------------------------------------------
class Operand:
    """a tensor living in the middle of a NaN-guarded device buffer"""

    def __init__(self, values, dtype, guard, shape=None):
        self.big, (self.guard, self.n) = nm.norm_guarded(values, guard, dtype, DEV)
        self.view = self.big[self.guard:self.guard + self.n].view(shape if shape is not None else tuple(values.shape))
        assert self.view.data_ptr() % 16 == 0
        self.before = self.bits().clone()

    def bits(self):
        return self.big.view(torch.int32 if self.big.dtype == torch.float32 else torch.int16)

    def unchanged(self):
        return torch.equal(self.bits(), self.before)

    def guards_intact(self):
        b, a = self.bits(), self.before
        return torch.equal(b[:self.guard], a[:self.guard]) and torch.equal(b[self.guard + self.n:], a[self.guard + self.n:])


def nan_operand(shape, dtype, guard):
    n = 1
    for s in shape:
        n *= s
    op = Operand(torch.zeros(n), dtype, guard, shape)
    op.bits()[:] = op.bits()[0]                # the slice too: never written = still NaN
    op.before = op.bits().clone()
    assert bool(torch.isnan(op.view).all())
    return op


def partials_guard(N, groups):
    return N * 8 * groups * 2


def gn_launch(c, dtype, n0=0, n1=None, counts=None, sets=None):
    """one ops.group_norm launch on samples [n0, n1) of case c, every operand guarded; returns (y [n, HW, 1, C] on the CPU as fp32, partials
    [n, 64, groups, 2] on the CPU, problems).  sets: the parameter sets to hand over (default: all of the case's)."""
    from edgestyle_amd import ops
    x = c["x"][n0:n1]
    n, HW, _, C = x.shape
    C1, C2, groups = c["C1"], c["C2"], c["groups"]
    sets = list(range(len(c["gamma"]))) if sets is None else sets
    xs = [Operand(x[..., :C1].contiguous(), dtype, GUARD)] + ([Operand(x[..., C1:].contiguous(), dtype, GUARD)] if C2 else [])
    gam = [Operand(c["gamma"][i], torch.float32, PGUARD) for i in sets]
    bet = [Operand(c["beta"][i], torch.float32, PGUARD) for i in sets]
    out = nan_operand((n, HW, 1, C), dtype, GUARD)
    part = nan_operand((n * nm.GN_MAX_CHUNK * groups * 2,), torch.float32, partials_guard(n, groups))
    for op, want in zip(xs, (x[..., :C1], x[..., C1:])):
        assert torch.equal(op.view.float().cpu(), want)
    grouped = len(sets) > 1
    y = ops.group_norm(xs[0].view, [g.view for g in gam] if grouped else gam[0].view, [b.view for b in bet] if grouped else bet[0].view, groups,
                       c["eps"], c["silu"], x2=xs[1].view if C2 else None, group_n=counts if grouped else None, out=out.view, partials=part.view)
    torch.cuda.synchronize()
    problems = []
    if y.data_ptr() != out.view.data_ptr():
        problems.append("out= was not used")
    for name, ops_ in (("x / x2", xs), ("gamma", gam), ("beta", bet)):
        if not all(o.unchanged() for o in ops_):
            problems.append(f"{name}: an input buffer was written")
    if not out.guards_intact():
        problems.append("a store outside out (guard no longer the NaN it was)")
    if not part.guards_intact():
        problems.append("a store outside partials (guard no longer NaN)")
    nan = int(torch.isnan(out.view).sum())
    if nan:
        problems.append(f"{nan} elements of out never written or NaN")
    route = gn_route_of(n, HW, C1, C2, groups)
    fin = torch.isfinite(part.view)
    rows = 0 if route["form"] == nm.GN_FORM_SLAB else route["nchunk"]
    lead = n * rows * groups * 2
    if not (bool(fin[:lead].all()) and not bool(fin[lead:].any())):
        problems.append(f"partials: {int(fin.sum())} finite floats, the route writes exactly the first {lead} ({rows} rows per sample)")
    return out.view.float().cpu(), part.view.cpu().reshape(n, nm.GN_MAX_CHUNK, groups, 2), problems


def gn_route_of(N, HW, C1, C2, groups, stats_only=False):
    from edgestyle_amd import lib
    return lib.group_norm_route(N, HW, C1, C2, groups, stats_only=stats_only)


def assert_route(row, route):
    """the library's route is the declared one, field for field the mirror's"""
    want = nm.gn_route(N_ROW, row["HW"], row["C1"] + row["C2"], row["groups"])
    assert route == want, (gn_id(row), route, want)
    assert route_class(route) == row["cls"] and all(route[k] == v for k, v in row["route"].items())


def act64(beta, silu):
    b = beta.double()
    return F.silu(b) if silu else b


def gn_run_row(row, dtype):
    fails = []
    name = f"norm gn {gn_id(row)} {T._name(dtype)}"
    c = nm.norm_case(row["HW"], row["C1"], row["C2"], row["groups"], N_ROW, row["kind"], dtype, silu=row["silu"], seed=row["seed"])
    route = gn_route_of(N_ROW, row["HW"], row["C1"], row["C2"], row["groups"])
    assert_route(row, route)
    y, _, problems = gn_launch(c, dtype)
    y2, _, p2 = gn_launch(c, dtype)
    fails += [f"{name}: {p}" for p in problems + p2]
    if not torch.equal(y, y2):
        fails.append(f"{name}: the same launch twice differs in {nm.differs(y, y2, count=True)} elements")
    for n in range(N_ROW):
        y1, _, p1 = gn_launch(c, dtype, n, n + 1)
        fails += [f"{name} sample {n} alone: {p}" for p in p1]
        if not torch.equal(y1[0], y[n]):
            fails.append(f"{name}: sample {n} launched alone differs from the N = {N_ROW} launch in {nm.differs(y1[0], y[n], count=True)} elements")
    ref = nm.gn_ref64(c)
    e_alg, e_ref = nm.row_err(nm.gn_base_alg(c, geom=route), ref), nm.row_err(nm.gn_base_ref(c), ref)
    judge(fails, name, y, ref, e_alg, e_ref, dtype)
    RECORD.append(dict(case=name, route=route_class(route), kernel=nm.row_err(y, ref), base_alg=e_alg, base_ref=e_ref, old_metric=nm.old_metric(y, ref)))
    if row["kind"] == "zero" and T.RECORD is None:
        want = nm.rnd(act64(c["beta"][0], row["silu"]), dtype).expand(row["HW"], 1, -1)
        if not torch.equal(y[0], want):
            fails.append(f"{name}: a zero sample must give the rounded act(beta) exactly; {nm.differs(y[0], want, count=True)} elements differ")
    return fails


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T._name)
@pytest.mark.parametrize("row", GN_TABLE, ids=gn_id)
def test_group_norm_on_every_route(row, dtype):
    """one table row: guarded operands, the declared route, twice the same bits, N = 3 equal to three N = 1 launches, the bars"""
    done(gn_run_row(row, dtype))


def test_table_coverage_is_printed():
    matrix, missing = coverage()
    print(f"test_norm_gpu: {len(GN_TABLE)} GroupNorm rows, {len(LN_TABLE)} LayerNorm rows\n{matrix}")
    assert not missing


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T._name)
@pytest.mark.parametrize("counts", [[1, 2], [1, 1, 2, 1]], ids=str)
@pytest.mark.parametrize("geo", GN_GROUPED, ids=lambda g: f"HW{g[0]}-C{g[1]}+{g[2]}-G{g[3]}")
def test_grouped_group_norm_equals_per_set_launches(geo, counts, dtype):
    """a grouped launch (one parameter set per run of samples) bit for bit its per-set launches, and inside the bars"""
    HW, C1, C2, groups, cls = geo
    N = sum(counts)
    c = nm.norm_case(HW, C1, C2, groups, N, "ratio_30", dtype, silu=True, counts=counts, seed=HW + N)
    route = gn_route_of(N, HW, C1, C2, groups)
    assert route_class(route) == cls and route == nm.gn_route(N, HW, C1 + C2, groups)
    name = f"norm gn grouped {counts} HW{HW} C{C1}+{C2} G{groups} {T._name(dtype)}"
    y, _, problems = gn_launch(c, dtype, counts=counts)
    fails = [f"{name}: {p}" for p in problems]
    a = 0
    for i, n in enumerate(counts):
        yi, _, pi = gn_launch(c, dtype, a, a + n, sets=[i])
        fails += [f"{name} set {i}: {p}" for p in pi]
        if not torch.equal(yi, y[a:a + n]):
            fails.append(f"{name}: set {i} launched alone differs in {nm.differs(yi, y[a:a + n], count=True)} elements")
        a += n
    ref = nm.gn_ref64(c, counts)
    e_alg, e_ref = nm.row_err(nm.gn_base_alg(c, counts, geom=route), ref), nm.row_err(nm.gn_base_ref(c, counts), ref)
    judge(fails, name, y, ref, e_alg, e_ref, dtype)
    done(fails)


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T._name)
@pytest.mark.parametrize("geo", GN_STATS_ONLY, ids=lambda g: f"HW{g[0]}-C{g[1]}-G{g[2]}")
def test_stats_only_sums_are_inside_the_standard_bound(geo, dtype):
    """es_group_norm(stats_only = 1): every written row of `partials` holds (sum x, sum x^2) of its (sample, chunk, group) with
    |S - S64| <= h 2^-24 sum|x| (and the same with x^2: the squares of fp16 / bf16 values are exact in fp32), h = nm.gn_sum_chain: the longest
    chain of fp32 additions on the route.  Exactly nchunk rows per sample are written, nothing else, and the launch repeats bit for bit."""
    from edgestyle_amd import lib, ops
    HW, C, groups = geo
    N, cpg = N_ROW, C // groups
    c = nm.norm_case(HW, C, 0, groups, N, "ratio_30", dtype, seed=HW)
    route = gn_route_of(N, HW, C, 0, groups, stats_only=True)
    assert route == nm.gn_route(N, HW, C, groups, stats_only=True) and route["form"] == nm.GN_FORM_TWO and route["blocks"] == 0
    two = nm.gn_route(N, HW, C, groups)
    assert (route["ppb"], route["nchunk"], route["ps"], route["lanes"]) == (two["ppb"], two["nchunk"], two["ps"], two["lanes"])
    nchunk, ppb = route["nchunk"], route["ppb"]
    got = []
    for _ in range(2):
        x = Operand(c["x"], dtype, GUARD)
        part = nan_operand((N * nm.GN_MAX_CHUNK * groups * 2,), torch.float32, partials_guard(N, groups))
        d = lib.GnDesc()
        d.x, d.partials = x.view.data_ptr(), part.view.data_ptr()
        d.N, d.HW, d.C1, d.C2, d.groups = N, HW, C, 0, groups
        d.eps, d.dtype, d.stats_only = 1e-5, ops._dt(x.view), 1
        lib.check(lib.load().es_group_norm(ctypes.byref(d), ops._stream()), "es_group_norm")
        torch.cuda.synchronize()
        assert x.unchanged() and part.guards_intact()
        fin = torch.isfinite(part.view)
        lead = N * nchunk * groups * 2
        assert bool(fin[:lead].all()) and not bool(fin[lead:].any()), (int(fin.sum()), lead)
        got.append(part.view[:lead].cpu().reshape(N, nchunk, groups, 2))
    assert torch.equal(got[0], got[1])
    xd = c["x"].double().reshape(N, HW, groups, cpg)
    xd = torch.cat([xd, torch.zeros(N, nchunk * ppb - HW, groups, cpg, dtype=torch.float64)], 1).reshape(N, nchunk, ppb, groups, cpg)
    h = nm.gn_sum_chain(route, cpg)
    fails = []
    for k, (name, v) in enumerate((("sum x", xd), ("sum x^2", xd * xd))):
        s64, mag = v.sum(dim=(2, 4)), v.abs().sum(dim=(2, 4))
        err = (got[0][..., k].double() - s64).abs()
        bound = h * 2.0 ** -24 * mag
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"norm stats_only HW{HW} C{C} G{groups} {T._name(dtype)}: {name}: h = {h}, largest |S - S64| / bound = {worst:.3f}")
        if not bool((err <= bound).all()):
            fails.append(f"{name}: |S - S64| exceeds h 2^-24 sum|x| (h = {h}) by a factor of {worst:.2f}")
    done(fails)


# ----------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------
def ln_launch(c, dtype, r0=0, r1=None, rows=None, sets=None):
    from edgestyle_amd import ops
    x = c["x"][r0:r1]
    sets = list(range(len(c["gamma"]))) if sets is None else sets
    xo = Operand(x, dtype, GUARD)
    gam = [Operand(c["gamma"][i], torch.float32, PGUARD) for i in sets]
    bet = [Operand(c["beta"][i], torch.float32, PGUARD) for i in sets]
    out = nan_operand(tuple(x.shape), dtype, GUARD)
    grouped = len(sets) > 1
    y = ops.layer_norm(xo.view, [g.view for g in gam] if grouped else gam[0].view, [b.view for b in bet] if grouped else bet[0].view, c["eps"],
                       group_rows=rows if grouped else None, out=out.view)
    torch.cuda.synchronize()
    problems = []
    if y.data_ptr() != out.view.data_ptr():
        problems.append("out= was not used")
    if not (xo.unchanged() and all(o.unchanged() for o in gam + bet)):
        problems.append("an input buffer was written")
    if not out.guards_intact():
        problems.append("a store outside out")
    nan = int(torch.isnan(out.view).sum())
    if nan:
        problems.append(f"{nan} elements of out never written or NaN")
    return out.view.float().cpu(), problems


def ln_run_row(row, dtype):
    from edgestyle_amd import lib
    M, C = row["M"], row["C"]
    name = f"norm ln {ln_id(row)} {T._name(dtype)}"
    assert lib.load().es_layer_norm_route(C) == LN_VPL[C]
    c = nm.ln_plain_case(nm.token_rows(M, C, row["ratio"], dtype=dtype, seed=M + C), dtype, seed=C)
    y, problems = ln_launch(c, dtype)
    y2, p2 = ln_launch(c, dtype)
    fails = [f"{name}: {p}" for p in problems + p2]
    if not torch.equal(y, y2):
        fails.append(f"{name}: the same launch twice differs")
    for r in range(M):                         # a row does not depend on its position in a 4-row block or on its neighbours
        y1, p1 = ln_launch(c, dtype, r, r + 1)
        fails += [f"{name} row {r} alone: {p}" for p in p1]
        if not torch.equal(y1[0], y[r]):
            fails.append(f"{name}: row {r} launched alone differs")
    ref = nm.ln_plain_ref64(c)
    e_alg, e_ref = nm.row_err(nm.ln_plain_base_alg(c), ref), nm.row_err(nm.ln_plain_base_ref(c), ref)
    judge(fails, name, y, ref, e_alg, e_ref, dtype)
    RECORD.append(dict(case=name, route=f"VPL {LN_VPL[C]}", kernel=nm.row_err(y, ref), base_alg=e_alg, base_ref=e_ref, old_metric=nm.old_metric(y, ref)))
    return fails


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T._name)
@pytest.mark.parametrize("row", LN_TABLE, ids=ln_id)
def test_layer_norm_on_every_instantiation(row, dtype):
    done(ln_run_row(row, dtype))


def test_layer_norm_refuses_a_row_no_instantiation_holds():
    """C = 4104 needs nine 16-byte chunks per lane: refused by name before anything is launched, out untouched"""
    from edgestyle_amd import ops, lib
    assert lib.load().es_layer_norm_route(4104) == 0 and lib.load().es_layer_norm_route(4096) == 8
    x = Operand(torch.ones(3, 4104), torch.float16, GUARD)
    out = nan_operand((3, 4104), torch.float16, GUARD)
    gam, bet = torch.ones(4104, device=DEV), torch.zeros(4104, device=DEV)
    with pytest.raises(lib.EdgeStyleHipError, match="4096 unsupported"):
        ops.layer_norm(x.view, gam, bet, out=out.view)
    torch.cuda.synchronize()
    assert out.unchanged()
    rc = lib.load().es_layer_norm(x.view.data_ptr(), out.view.data_ptr(), gam.data_ptr(), bet.data_ptr(), 3, 4104, 1e-5, lib.ES_F16, ops._stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"C > 4096 unsupported" in lib.load().es_last_error() and out.unchanged()


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T._name)
@pytest.mark.parametrize("C", [8, 520, 1032, 1544, 4096])
def test_grouped_layer_norm_with_set_boundaries_inside_row_blocks(C, dtype):
    """rows [3, 6, 1, 3]: the sets end at rows 3, 9 and 10, all inside 4-row workgroups.  Bit for bit the per-set launches; inside the bars."""
    rows = [3, 6, 1, 3]
    M = sum(rows)
    c = nm.ln_plain_case(nm.token_rows(M, C, 30, dtype=dtype, seed=C), dtype, ngroups=4, seed=C)
    name = f"norm ln grouped {rows} C{C} {T._name(dtype)}"
    y, problems = ln_launch(c, dtype, rows=rows)
    fails = [f"{name}: {p}" for p in problems]
    a = 0
    for i, n in enumerate(rows):
        yi, pi = ln_launch(c, dtype, a, a + n, sets=[i])
        fails += [f"{name} set {i}: {p}" for p in pi]
        if not torch.equal(yi, y[a:a + n]):
            fails.append(f"{name}: set {i} launched alone differs")
        a += n
    ref = nm.ln_plain_ref64(c, rows)
    e_alg, e_ref = nm.row_err(nm.ln_plain_base_alg(c, rows), ref), nm.row_err(nm.ln_plain_base_ref(c, rows), ref)
    judge(fails, name, y, ref, e_alg, e_ref, dtype)
    done(fails)


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T._name)
@pytest.mark.parametrize("C", [8, 520, 1032, 1544, 2056, 4096])
def test_layer_norm_constant_and_zero_rows_give_beta(C, dtype):
    """The statistics are an exact two-pass: on a row of one value v (k v is exact in fp32 for k <= 4096 and 11-bit v) the mean is v, every
    deviation is 0 and the output is the rounded beta - bit for bit; the rows next to it are ordinary ones and stay inside the bars."""
    M = 5
    x = nm.token_rows(M, C, 0, dtype=dtype, seed=C + 1)
    x[1] = nm.NORM_CONSTANT
    x[3] = 0.0
    c = nm.ln_plain_case(x, dtype, seed=C)
    y, problems = ln_launch(c, dtype)
    fails = list(problems)
    want = nm.rnd(c["beta"][0], dtype)
    for r in (1, 3):
        if not torch.equal(y[r], want):
            fails.append(f"row {r} (one value): {nm.differs(y[r], want, count=True)} elements are not the rounded beta")
        assert torch.equal(nm.ln_plain_base_alg(c)[r], want)
    ref = nm.ln_plain_ref64(c)
    judge(fails, f"norm ln one-value rows C{C} {T._name(dtype)}", y, ref, nm.row_err(nm.ln_plain_base_alg(c), ref), nm.row_err(nm.ln_plain_base_ref(c), ref), dtype)
    done(fails)


def report_rows():
    """python -m tests.numerics --report --only norm: run every row without asserting, return (records, seconds)"""
    del RECORD[:]
    t0 = time.time()
    for dtype in T.DTYPES:
        for row in GN_TABLE:
            gn_run_row(row, dtype)
        for row in LN_TABLE:
            ln_run_row(row, dtype)
    return list(RECORD), time.time() - t0
