"""es_linear_xs (csrc/linear_xs.hip) in every instantiation, at every stage count its counted waits branch on and at every ragged edge,
judged per row against fp64 (tests/numerics.py, the xs section; method: tests/NUMERICS.md).

launch() of linear_xs.hip picks one of 16 kernels per dtype (nm.XS_FORMS): the one-barrier form at K = 320 plain | LN | GEGLU | GEGLU+LN |
residual and K = 640 plain | LN | GEGLU | GEGLU+LN, the ping-pong form at K = 320 plain | LN | residual | GN and K = 640 plain | LN | GN.  TABLE
is no cross product: every form meets every class `coverage()` names - lines per slice 1 .. 7 (P = 1), 1 .. 4 (P = 2), 1 .. 3 (P = 4), one run
of 12 lines and more, one uneven split with a short last slice; M in XS_MS (GN forms: hw 256 | 512, N 1 | 3, every group count); grouped
launches of two, three and four weight sets, one with a ragged last run - and `coverage()` is asserted at import.  Every row runs in fp16
and bf16.

A row is launched three times in one process: dense, through views into NaN-filled buffers (x a row slice between NaN rows; out and the
residual slices of pitch cstore + 64 with 256 guard rows on either side), dense again.  The three payloads are equal bit for bit, every
guard keeps its NaN bits, the payload holds no NaN, es_linear_xs_last_form() names the row's instantiation, the recorded descriptor holds
the slices the row asks for, and - forms without GEGLU and GN - the other setting of es_linear_xs_set_pp gives the same bits on the form
that differs in the PP bit alone.  Bars: row_err <= 2 x base_alg, <= 2 x base_ref, finite where the rounded reference is; plain and
GEGLU-without-LN rows also the misrounded share against chains of 8, chains of 32 and torch fp32; residual rows `differs` from base_alg."""
import ctypes
import time

import pytest
import torch

from tests import numerics as nm
from tests import test_numerics_gpu as T
from tests.test_numerics_gpu import judge, done, knobs, launches

pytestmark = pytest.mark.gpu

DEV = "cuda"
RECORD = []                     # one dict per judged row (python -m tests.numerics --report --only xs writes them to NUMERICS.md)
XS_MS = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 256 + 129, 3 * 256)
XS_GROUPED = ([256, 512], [256, 256, 256], [256, 256, 256, 256], [256, 129])     # (four sets need 1024 rows: the one launch above 768)
XS_MAX_LINES = 24
NMAX = {1: 7, 2: 4, 4: 3}       # lines per slice up to which every count is a class of its own, by stages per line
# GroupNorm in front: (hw, N, groups, counts); 5 groups at K = 320 only
GN_GEOMS = {320: [(256, 1, 32, None), (256, 3, 1, None), (512, 1, 2, None), (256, 3, 5, [1, 2]), (512, 1, 32, None), (256, 1, 5, None),
                  (256, 3, 32, None), (512, 1, 1, None), (256, 1, 2, None)],
            640: [(256, 1, 32, None), (256, 3, 1, None), (512, 1, 2, None), (256, 3, 32, [1, 2]), (512, 1, 1, None), (256, 1, 2, None)]}


def stage_classes(P):
    """(lines, slices) per class: n lines per slice for n = 1 .. NMAX (odd n: one slice; even n: two), a long run, an uneven split"""
    out = [(n, 1) if n % 2 else (2 * n, 2) for n in range(1, NMAX[P] + 1)]
    out.append((13, 1) if P == 1 else (12, 1))
    out.append((7, 3) if P == 1 else (5, 2))                       # 3 + 3 + 1 and 3 + 2
    return out


def build_table():
    rows = []
    for K, kind, pp in nm.XS_FORMS:
        P = nm.xs_geometry(K, kind)[2]
        sc = stage_classes(P)
        if kind == "gn":
            geoms = GN_GEOMS[K]
            for i in range(max(len(sc), len(geoms))):
                hw, N, G, counts = geoms[i % len(geoms)]
                lines, slices = sc[i % len(sc)]
                rows.append(dict(K=K, kind=kind, pp=pp, M=N * hw, lines=lines, slices=slices, counts=counts, hw=hw, N=N, G=G, ratio=(0, 30)[i % 2]))
            continue
        for i, M in enumerate(XS_MS):
            lines, slices = sc[i % len(sc)]
            rows.append(dict(K=K, kind=kind, pp=pp, M=M, lines=lines, slices=slices, counts=None, ratio=(0, 30)[i % 2]))
        for i, counts in enumerate(XS_GROUPED):
            lines, slices = sc[(i + 1) % len(sc)]
            rows.append(dict(K=K, kind=kind, pp=pp, M=sum(counts), lines=lines, slices=slices, counts=counts, ratio=(30, 0)[i % 2]))
    for i, r in enumerate(rows):
        r["seed"] = 7 * i + 3
    return rows


TABLE = build_table()


def form_name(K, kind, pp):
    return f"K{K}-{kind}-{'pp' if pp else '1b'}"


def row_id(r):
    g = "" if r["counts"] is None else "-sets" + "+".join(str(n) for n in r["counts"])
    gn = f"-hw{r['hw']}-N{r['N']}-G{r['G']}" if r["kind"] == "gn" else ""
    return f"{form_name(r['K'], r['kind'], r['pp'])}-M{r['M']}-L{r['lines']}-S{r['slices']}{gn}{g}"


def row_split(r):
    """(nslices, chunks_per_slice, stages of the last slice) the row's launch must record"""
    return nm.xs_split(r["lines"], r["slices"], nm.xs_geometry(r["K"], r["kind"])[2])


def coverage():
    """form -> the classes its rows meet; returns (text, the unmet cells)"""
    lines, missing = [], []
    for form in nm.XS_FORMS:
        K, kind, pp = form
        P = nm.xs_geometry(K, kind)[2]
        rows = [r for r in TABLE if (r["K"], r["kind"], r["pp"]) == form]
        splits = [row_split(r) for r in rows]
        per_slice = {cps // P for _, cps, _ in splits}
        nch = sorted({cps for _, cps, _ in splits} | {last for _, _, last in splits})
        need = [("lines per slice", n) for n in range(1, NMAX[P] + 1) if n not in per_slice]
        if not any(cps // P >= 12 for _, cps, _ in splits):
            need.append(("a run of 12 lines", None))
        if not any(ns > 1 and last < cps for ns, cps, last in splits):
            need.append(("a short last slice", None))
        if kind == "gn":
            need += [("hw", v) for v in (256, 512) if not any(r["hw"] == v for r in rows)]
            need += [("N", v) for v in (1, 3) if not any(r["N"] == v for r in rows)]
            need += [("groups", v) for v in ((32, 1, 2, 5) if K == 320 else (32, 1, 2)) if not any(r["G"] == v for r in rows)]
            if not any(r["counts"] == [1, 2] for r in rows):
                need.append(("counts", [1, 2]))
            what = f"hw x N x G {sorted({(r['hw'], r['N'], r['G']) for r in rows})}"
        else:
            need += [("M", m) for m in XS_MS if not any(r["M"] == m and r["counts"] is None for r in rows)]
            sets = [r["counts"] for r in rows if r["counts"]]
            need += [("weight sets", n) for n in (2, 3, 4) if not any(len(c) == n and all(v % 256 == 0 for v in c) for c in sets)]
            need += [("a run of rows", v) for v in (256, 512) if not any(v in c for c in sets)]
            if not any(c[-1] % 256 for c in sets):
                need.append(("a ragged last run", None))
            what = f"M {sorted({r['M'] for r in rows})} sets {sets}"
        missing += [(form_name(*form), n) for n in need]
        lines.append(f"{form_name(*form):<18} P {P}  {len(rows):>2} rows  lines/slice {sorted(per_slice)}  stages per workgroup {nch}  {what}")
    return "\n".join(lines), missing


_matrix, _missing = coverage()
assert not _missing, f"test_linear_xs_gpu.TABLE leaves unmet: {_missing}\n{_matrix}"
assert len({row_id(r) for r in TABLE}) == len(TABLE)
assert all(r["lines"] <= XS_MAX_LINES and (r["M"] <= 768 or r["counts"] == [256] * 4) for r in TABLE)
assert {(r["K"], r["kind"], r["pp"]) for r in TABLE} == set(nm.XS_FORMS) and len(nm.XS_FORMS) == 16


# ----------------------------------------------------------------------------------------------------------------
# launching
# ----------------------------------------------------------------------------------------------------------------
def nan_rows(t, guard, dtype):
    """(buffer, middle slice) of a 2-d operand between `guard` rows of payload NaNs"""
    M, C = t.shape
    big = torch.full((M + 2 * guard, C), nm.ATTN_NAN_BITS[dtype], dtype=torch.int16).view(dtype)
    big[guard:guard + M] = t.to(dtype)
    big = big.to(DEV)
    return big, big[guard:guard + M]


def pack(c):
    """the case's weight sets as ops packs them"""
    from edgestyle_amd import ops
    dt = c["dtype"]
    if c["kind"] == "gn":
        g = c["gn"]
        return [ops.pack_weight(w, b, dt, DEV) for w, b in zip(g["W"], g["b"])]
    out = []
    for q in c["sets"]:
        if q["ln"]:
            out.append(ops.pack_weight_ln(q["W"], q["b"], q["gamma"], q["beta"], q["eps"], dt, DEV, geglu=q["geglu"]))
        else:
            out.append(ops.pack_weight(q["W"], q["b"], dt, DEV, geglu=q["geglu"]))
    return out


def gn_stats(c, x):
    """the statistics exactly as ops.gn_proj_in produces them: es_group_norm(stats_only) on the raw tensor"""
    from edgestyle_amd import ops, lib
    N, hw, G = c["N"], c["hw"], c["G"]
    part = ops._gn_partials_for("test_linear_xs", x, N, G)
    d = lib.GnDesc()
    d.x, d.partials = x.data_ptr(), part.data_ptr()
    d.N, d.HW, d.C1, d.C2, d.groups = N, hw, c["K"], 0, G
    d.eps, d.silu, d.dtype, d.stats_only = 1e-6, 0, ops._dt(x), 1
    lib.check(lib.load().es_group_norm(ctypes.byref(d), ops._stream()), "es_group_norm")
    g = c["gn"]
    return dict(part=part, gamma=[t.to(DEV) for t in g["gamma"]], beta=[t.to(DEV) for t in g["beta"]], groups=G,
                nchunk=lib.load().es_group_norm_chunks(hw), hw=hw, eps=1e-6)


def launch(c, pws, slices, guarded):
    """one ops.linear_xs launch of case c; returns (payload on the CPU as fp32, the recorded descriptor's (nslices, chunks_per_slice, ldo),
    es_linear_xs_last_form, problems)"""
    from edgestyle_amd import ops, lib
    dt, M, cstore = c["dtype"], c["M"], c["cstore"]
    problems = []
    if guarded:
        xbig, x = nan_rows(c["x"], 8, dt)
        obig, out = nm.xs_out_guarded(M, cstore, dt, DEV)
        rbig = res = None
        if c["kind"] == "res":
            rbig, res = nm.xs_out_guarded(M, cstore, dt, DEV)
            res.copy_(c["res"].to(DEV, dt))
            rbefore = rbig.view(torch.int16).clone()
        xbefore = xbig.view(torch.int16).clone()
        assert x.is_contiguous() and x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and (M == 1 or out.stride(0) == cstore + nm.XS_PAD_COLS)
    else:
        x = c["x"].to(DEV, dt)
        out = torch.full((M, cstore), nm.ATTN_NAN_BITS[dt], dtype=torch.int16).view(dt).to(DEV)
        res = c["res"].to(DEV, dt) if c["kind"] == "res" else None
    gn = rows = None
    if c["kind"] == "gn":
        gn = gn_stats(c, x.reshape(c["N"], c["hw"], 1, c["K"]))
        rows = None if c["counts"] is None else [n * c["hw"] for n in c["counts"]]
    elif c["counts"] is not None:
        rows = c["counts"]
    with knobs(XS_FORCE_SLICES=slices), launches() as rec:
        ops.linear_xs(x, pws if len(pws) > 1 else pws[0], M, out, rows, residual=res, gn=gn)
    form = lib.load().es_linear_xs_last_form()
    torch.cuda.synchronize()
    d = [d for d in rec.descs if isinstance(d, lib.XsDesc)]
    assert len(d) == 1
    if guarded:
        if not nm.xs_guards_intact(obig, M, cstore):
            problems.append("a store outside out (a guard row or guard column is no longer the NaN it was)")
        if not torch.equal(xbig.view(torch.int16), xbefore):
            problems.append("x was written")
        if rbig is not None and not torch.equal(rbig.view(torch.int16), rbefore):
            problems.append("the residual was written")
    nan = int(torch.isnan(out).sum())
    if nan:
        problems.append(f"{nan} elements of out never written or NaN")
    return out.float().cpu(), (d[0].nslices, d[0].chunks_per_slice, d[0].ldo), form, problems


def judge_shares(fails, name, c, y, ref, base):
    """plain / GEGLU rows: the misrounded share against the independent fp32 baselines; residual rows: `differs` from base_alg"""
    dt = c["dtype"]
    if c["kind"] == "res":
        counts = {k: nm.differs(v, base["alg8"], count=True) for k, v in base.items() if k != "alg8"}
        n_kernel, against = nm.differs(y, base["alg8"], count=True), "base_alg"
    else:
        counts = {k: nm.misrounded(v, ref, dt, count=True) for k, v in base.items()}
        n_kernel, against = nm.misrounded(y, ref, dt, count=True), "the rounded fp64 result"
    numel = ref.numel()
    bar = nm.misrounded_bar(counts.values())
    small = "" if numel >= nm.CONV_MIN_ELEMENTS else f" [{numel} elements: under {nm.CONV_MIN_ELEMENTS}, the floor of {nm.MISROUNDED_FLOOR} is loose here]"
    print(f"numerics: {name}: differing from {against}: kernel {n_kernel} ({n_kernel / numel:.4%})  baselines "
          + " ".join(f"{k} {v / numel:.4%}" for k, v in counts.items()) + f"  bar {bar}{small}", flush=True)
    if T.RECORD is None and n_kernel > bar:
        fails.append(f"{name}: {n_kernel} elements differ from {against}, the bar is {bar} ({counts})")
    return n_kernel, bar


def run_row(r, dtype):
    from edgestyle_amd import lib
    L = lib.load()
    K, kind, pp = r["K"], r["kind"], r["pp"]
    name = f"xs {row_id(r)} {T._name(dtype)}"
    fails = []
    kw = dict(hw=r["hw"], G=r["G"], N=r["N"]) if kind == "gn" else {}
    c = nm.xs_case(r["M"], K, r["lines"], kind, dtype, seed=r["seed"], counts=r["counts"], ratio=r["ratio"], **kw)
    pws = pack(c)
    want_form = nm.xs_form_id(K, kind, pp)
    want_split = row_split(r)[:2]
    switchable = kind in ("plain", "ln", "res")          # the forms es_linear_xs_set_pp chooses between
    prev = L.es_linear_xs_set_pp(pp if switchable else 1)
    try:
        runs = [launch(c, pws, r["slices"], guarded) for guarded in (False, True, False)]
        if switchable:
            L.es_linear_xs_set_pp(1 - pp)
            twin = launch(c, pws, r["slices"], False)
    finally:
        L.es_linear_xs_set_pp(prev)
    y = runs[0][0]
    for tag, (yi, (ns, cps, ldo), form, problems) in zip(("dense", "views", "dense again"), runs):
        fails += [f"{name} {tag}: {p}" for p in problems]
        if form != want_form:
            fails.append(f"{name} {tag}: ran on form {form:#x}, the row names {want_form:#x}")
        if (ns, cps) != want_split:
            fails.append(f"{name} {tag}: recorded {ns} slices of {cps} stages, the row asks for {want_split}")
        if ldo != (c["cstore"] + nm.XS_PAD_COLS if tag == "views" and r["M"] > 1 else c["cstore"]):
            fails.append(f"{name} {tag}: recorded pitch {ldo}")
        if not torch.equal(yi, y):
            fails.append(f"{name}: {tag} differs from the dense launch in {nm.differs(yi, y, count=True)} elements")
    if switchable:
        yt, _, form_t, problems = twin
        fails += [f"{name} other form: {p}" for p in problems]
        if form_t != want_form ^ nm.XS_FORM_PP:
            fails.append(f"{name}: es_linear_xs_set_pp({1 - pp}) ran form {form_t:#x}, not {want_form ^ nm.XS_FORM_PP:#x}")
        if not torch.equal(yt, y):
            fails.append(f"{name}: the two forms differ in {nm.differs(yt, y, count=True)} elements")
    ref = nm.xs_ref64(c)
    alg8 = nm.xs_base_alg(c, 8)
    e_alg, e_ref = nm.row_err(alg8, ref), nm.row_err(nm.xs_base_ref(c), ref)
    judge(fails, name, y, ref, e_alg, e_ref, dtype)
    rec = dict(case=name, form=f"{want_form:#x}", kernel=nm.row_err(y, ref), base_alg=e_alg, base_ref=e_ref, old_metric=nm.old_metric(y, ref),
               differs=None, bar=None, numel=ref.numel())
    if nm.xs_rounds_once(kind) or kind == "res":
        base = {"alg8": alg8, "alg32": nm.xs_base_alg(c, 32), "torch32": nm.xs_base_alg(c, None)}
        rec["differs"], rec["bar"] = judge_shares(fails, name, c, y, ref, base)
    RECORD.append(rec)
    return fails


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T._name)
@pytest.mark.parametrize("row", TABLE, ids=row_id)
def test_linear_xs_in_every_form(row, dtype):
    """one table row: dense, through NaN-guarded pitched views, dense again - the same bits, the form and slices the row names, both
    ping-pong settings where the form has two, the fp64 bars"""
    done(run_row(row, dtype))


def test_table_coverage_is_printed():
    matrix, missing = coverage()
    print(f"test_linear_xs_gpu: {len(TABLE)} rows in {len(nm.XS_FORMS)} forms, two dtypes each\n{matrix}")
    assert not missing


# ----------------------------------------------------------------------------------------------------------------
# routed through ops.linear and ops.gn_proj_in
# ----------------------------------------------------------------------------------------------------------------
ROUTED = [(320, "plain", 300), (320, "res", 257), (320, "geglu", 130), (640, "ln", 200), (640, "geglu_ln", 33)]


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T._name)
@pytest.mark.parametrize("K,kind,M", ROUTED, ids=lambda v: str(v))
def test_ops_linear_routes_the_smallest_eligible_widths_to_linear_xs(K, kind, M, dtype):
    """ops.linear with XS_MIN_M = 0 at the smallest width it lets through (four output lines): the route is linear_xs, the bars hold"""
    from edgestyle_amd import ops, lib
    c = nm.xs_case(M, K, 4, kind, dtype, seed=K + M, ratio=30)
    pw = pack(c)[0]
    x = c["x"].to(DEV, dtype)
    res = c["res"].to(DEV, dtype) if kind == "res" else None
    with knobs(XS_ENABLED=True, XS_MIN_M=0), launches() as rec:
        y = ops.linear(x, pw, residual=res) if res is not None else ops.linear(x, pw)
    assert len(rec.descs) == 1 and isinstance(rec.descs[0], lib.XsDesc), "not routed to linear_xs"
    ref = nm.xs_ref64(c)
    fails = []
    judge(fails, f"xs routed ops.linear K{K} {kind} M{M} {T._name(dtype)}", y, ref, nm.row_err(nm.xs_base_alg(c, 8), ref), nm.row_err(nm.xs_base_ref(c), ref), dtype)
    done(fails)


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T._name)
@pytest.mark.parametrize("G,counts", [(32, None), (5, [16, 16])], ids=lambda v: str(v))
def test_ops_gn_proj_in_routes_the_smallest_eligible_launch_to_linear_xs(G, counts, dtype):
    """ops.gn_proj_in folds the GroupNorm into the projection from 8192 rows on at K = 320 (32768 at K = 640: the 8 x 64 x 64 case of
    test_numerics_gpu.py), whatever XS_MIN_M says: 32 maps of 16 x 16 and four output lines - one es_linear_xs launch with gn_part set, on
    the GN form, inside the bars"""
    from edgestyle_amd import ops, lib
    K, N, hw = 320, 32, 256
    c = nm.xs_case(N * hw, K, 4, "gn", dtype, seed=G, counts=counts, ratio=30, hw=hw, G=G, N=N)
    pws = pack(c)
    g = c["gn"]
    gam, bet = [t.to(DEV) for t in g["gamma"]], [t.to(DEV) for t in g["beta"]]
    x = c["x"].to(DEV, dtype).reshape(N, 16, 16, K)
    with knobs(XS_ENABLED=True, XS_MIN_M=0, GN_FOLD=True), launches() as rec:
        assert ops.gn_fold_ok(N * hw, hw, G, pws[0], pws if counts else None, counts)
        assert not ops.gn_fold_ok(N * hw - hw, hw, G, pws[0], None, None), "a smaller launch folds too: move this row there"
        y = ops.gn_proj_in(x, gam, bet, G, 1e-6, pws, group_n=counts) if counts else ops.gn_proj_in(x, gam[0], bet[0], G, 1e-6, pws[0])
    assert len(rec.descs) == 1 and isinstance(rec.descs[0], lib.XsDesc) and rec.descs[0].gn_part, "not routed to linear_xs with the GroupNorm in front"
    assert lib.load().es_linear_xs_last_form() == nm.xs_form_id(K, "gn", 1)
    ref = nm.xs_ref64(c)
    fails = []
    judge(fails, f"xs routed ops.gn_proj_in K{K} G{G} N{N}{' grouped' if counts else ''} {T._name(dtype)}", y.reshape(N * hw, -1), ref,
          nm.row_err(nm.xs_base_alg(c, 8), ref), nm.row_err(nm.xs_base_ref(c), ref), dtype)
    done(fails)


def report_rows():
    """python -m tests.numerics --report --only xs: run every row without asserting, return (records, seconds)"""
    del RECORD[:]
    t0 = time.time()
    for dtype in T.DTYPES:
        for row in TABLE:
            run_row(row, dtype)
    return list(RECORD), time.time() - t0
