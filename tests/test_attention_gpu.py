"""es_attention at ragged lengths, through poisoned views, into guarded outputs - every kernel the dispatcher can pick, against fp64.

test_numerics_gpu.py drives the seven attention variants with hard inputs at whole tiles; test_ops_gpu.py has the ragged shapes with randn,
dense operands and whichever kernel the dispatcher happens to pick.  Here the two meet.  Every row of TABLE is one problem on one asserted
kernel, launched three times in one child process (the dispatcher reads its switches once per process - the children of
test_numerics_gpu.py, extended):

    dense contiguous q, k, v into a plain `out`;
    q | k | v as column slices of one buffer whose every other element is a payload NaN, into an `out` view inside NaN guards;
    the same with the buffer's other elements at +-6e4 (fp16) / +-3e38 (bf16) - a multiply by a masked zero hides that, a max hides the NaN.

Asserted per row: the kernel that ran, all three times; the three outputs equal BIT FOR BIT (the kernels have no atomics and no arithmetic
that depends on a stride: a difference is a read outside a view); every guard element of both guarded buffers still holds its NaN bits
and the views hold none; kernel <= 2 base_alg and <= 2 base_ref against attn_ref64 (required tier), finite where the rounded reference is;
with one key, the output IS v[:, 0].

TABLE is no cross product: REQUIRED lists, per variant, the classes it has to meet (query raggedness against its workgroup and wave
sizes, key raggedness against its tile, input classes, dtypes, head widths, dispatcher edges); `coverage()` checks that, is asserted at
import and prints the matrix.  A variant's precondition shapes its rows, nothing is skipped at run time.  Which kernel a row goes to, and the
K/V-resident kernel's strips, are asked of nm.attn_route (the Python mirror of the library's route, held to it in tests/test_host_cpu.py);
test_attention_route_is_the_launch checks in this process that the kernel the library's route names is the kernel that then runs."""
import os
import subprocess
import sys
import time

import pytest
import torch

from tests import numerics as nm
from tests import test_numerics_gpu as T
from tests.test_numerics_gpu import ATTN_KERNELS, ATTN_KERNEL_ID, judge, done

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = T.ROOT
KINDS = nm.ATTN_INPUT_KINDS
ALL_WIDTHS = (8, 16, 24, 32, 40, 48, 64, 80, 128, 160, 512)        # ok_d of es_attention

# queries per workgroup (B) and per wave (w); two: a wave runs two 32-query blocks; keys: which key counts the variant takes
GEOMETRY = {
    "generic": dict(B=64, w=16, two=False, keys="tiled"),
    "generic_32q": dict(B=128, w=32, two=False, keys="tiled"),
    "tile32": dict(B=128, w=32, two=False, keys="tiled"),
    "tile32_2blocks": dict(B=256, w=64, two=True, keys="tiled"),
    "attention40pp_32q": dict(B=256, w=32, two=False, keys="pp"),
    "attention40pp_64q": dict(B=512, w=64, two=True, keys="pp"),
    "kv_resident": dict(B=None, w=None, two=False, keys="kvres"),
}
TILED_KEYS = (1, 63, 64, 65, 127, 129, 193)             # the tile is 64 keys, double-buffered, prefetched two tiles ahead
PP_KEYS = (128, 192, 320)                               # Skv % 64 == 0 and >= 128: odd and even tile counts for two groups one tile out of phase
KVRES_KEYS = (1, 5, 31, 32, 33, 64, 65, 77, 80, 81, 95, 96)     # every 32-key tile edge, and the short3 boundary at 80
KVRES_QUERIES = (64, 65, 95, 97)
KVRES_HEADS = (1, 6, 8, 9, 12)                          # 9: the second workgroup of eight heads has a single one


ENV_KNOB = dict(ES_ATTN32="attn32", ES_ATTN_BIG="big_thr", ES_ATTN_PP="pp", ES_ATTN_QB="qb")


def row_knobs(r, **kw):
    """the knobs a row's child runs under: its variant's environment and its own es_attention_set_kvres, as nm.attn_route takes them"""
    k = dict(nm.ATTN_KNOBS, kvres=r["kvres"], **{ENV_KNOB[name]: int(val) for name, val in ATTN_KERNELS[r["variant"]][0].items()})
    return dict(k, **kw)


def kvres_strips(N, heads, Sq):
    """the K/V-resident kernel's strip rule (nm.attn_route, the mirror of csrc/attention.hip's): (queries per strip, strips)"""
    route = nm.attn_route(N, heads, Sq, 77, 40, dict(nm.ATTN_KNOBS, kvres=2))
    assert route["kernel"] == ATTN_KERNEL_ID["kv_resident"]
    return route["qper"], route["grid_x"]


def _row(variant, Sq, Skv, kind, d=40, bf=False, N=2, heads=2, scale=None, kvres=None, expect=None, batch_slice=False, tag=()):
    assert kind in KINDS
    kvres = ATTN_KERNELS[variant][2] if kvres is None else kvres
    seed = 7 * Sq + 13 * Skv + d + 1000 * KINDS.index(kind) + (500 if bf else 0) + heads      # recorded with the row (and printed)
    return dict(variant=variant, expect=expect or variant, N=N, heads=heads, Sq=Sq, Skv=Skv, d=d, bf=bool(bf), kind=kind, seed=seed,
                scale=scale, kvres=kvres, batch_slice=batch_slice, tag=tuple(tag))


def _sq(sqs, i, kind):
    """the i-th query length in turn; one_loud_query needs calm queries beside the loud one, so not a single query"""
    Sq = sqs[i % len(sqs)]
    return sqs[-1] if (Sq == 1 and kind == "one_loud_query") else Sq


def _tiled_rows(variant, widths):
    """the seven key counts against the variant's query lengths and the six input classes (one key: nothing for a softmax to decide)"""
    g = GEOMETRY[variant]
    B, w = g["B"], g["w"]
    sqs = [1, B - 1, B + 1, B + w + 1] + ([B + 64 + 17] if g["two"] else [])
    kinds = ["randn", "shift-300", "shift+300", "last_key_decides", "one_loud_query", "loud_values_2e4", "shift-300"]
    rows = [_row(variant, _sq(sqs, i, kinds[i]), Skv, kinds[i], d=widths[i % len(widths)], bf=i % 2 == 1) for i, Skv in enumerate(TILED_KEYS)]
    rows.append(_row(variant, sqs[-1], 65, "shift-300", d=widths[-1], bf=True))                 # one padded key short of a whole tile pair ...
    rows.append(_row(variant, sqs[1], 129, "last_key_decides", d=widths[0], bf=False, N=1, heads=3))
    return rows


def _pp_rows(variant):
    g = GEOMETRY[variant]
    B, w = g["B"], g["w"]
    sqs = [1, B - 1, B + 1, B + w + 1] + ([B + 64 + 17] if g["two"] else [])
    rows = [_row(variant, _sq(sqs, i, kind), PP_KEYS[i % 3], kind, bf=i % 2 == 1, N=1 + i % 2) for i, kind in enumerate(KINDS)]
    if g["two"]:
        rows.append(_row(variant, sqs[-1], 320, "shift-300", bf=True, N=1))
    # under the ping-pong switches a key count the kernel cannot take falls back to the tiled two-block kernel
    rows.append(_row(variant, B + 1, 127, "shift-300", expect="tile32_2blocks", tag=("fallback_k127",)))
    rows.append(_row(variant, 65, 64, "last_key_decides", bf=True, expect="tile32_2blocks", tag=("fallback_k64",)))
    return rows


def _kvres_rows():
    v = "kv_resident"
    kinds = ["randn"] + [KINDS[i % 6] for i in range(1, len(KVRES_KEYS))]
    rows = [_row(v, KVRES_QUERIES[i % 4], Skv, kinds[i], d=(40, 80)[i % 2], bf=i % 4 >= 2, N=1 + i % 3, heads=KVRES_HEADS[i % 5])
            for i, Skv in enumerate(KVRES_KEYS)]
    rows.append(_row(v, 97, 77, "shift-300", d=80, bf=True, N=2, heads=9))
    rows.append(_row(v, 65, 77, "last_key_decides", d=40, bf=False, N=3, heads=12))
    # a strip of more than one 32-query block whose last one is part-filled needs more workgroups per strip than N <= 3 gives: one head,
    # many samples (the reference stays tiny)
    rows.append(_row(v, 290, 77, "one_loud_query", d=40, N=32, heads=1, tag=("qper",)))
    # the dispatcher's edges (default switches: what is not KV-resident goes to the 16-queries-per-wave generic kernel)
    rows.append(_row(v, 64, 97, "shift-300", d=40, expect="generic", tag=("edge_Skv97",)))
    rows.append(_row(v, 63, 96, "shift-300", d=80, bf=True, expect="generic", tag=("edge_Sq63",)))
    rows.append(_row(v, 64, 77, "shift+300", d=40, N=12, heads=1, kvres=1, tag=("edge_groups12_d40",)))
    rows.append(_row(v, 64, 77, "shift+300", d=40, N=11, heads=1, kvres=1, expect="generic", tag=("edge_groups11_d40",)))
    rows.append(_row(v, 161, 77, "loud_values_2e4", d=80, bf=True, N=64, heads=1, kvres=1, tag=("edge_groups64_d80", "qper")))
    rows.append(_row(v, 64, 77, "randn", d=80, N=63, heads=1, kvres=1, expect="generic", tag=("edge_groups63_d80",)))
    return rows


def _width_rows(variant, widths):
    """every head width in both dtypes on the kernel dispatch() gives it, ragged on both sides"""
    rows = []
    for i, d in enumerate(widths):
        for bf in (False, True):
            Sq, Skv = (33, 45) if d == 512 else (70, 77)
            kind = KINDS[(i + bf) % 6]
            rows.append(_row(variant, Sq, Skv, kind, d=d, bf=bf, N=2, heads=1 if d >= 128 else 3, tag=("width",)))
    return rows


TABLE = (_tiled_rows("generic", (40, 80, 160)) + _width_rows("generic", ALL_WIDTHS)
         + [_row("generic", 70, 77, "randn", d=40, scale=0.2, tag=("scale",)),
            _row("generic", 65, 193, "shift-300", d=80, bf=True, N=3, batch_slice=True, tag=("batch_slice",)),
            _row("generic", 33, 45, "last_key_decides", d=512, N=1, heads=1), _row("generic", 17, 31, "shift-300", d=512, bf=True, N=1, heads=1)]
         + _tiled_rows("generic_32q", (40, 80)) + _width_rows("generic_32q", (40, 48, 80))
         + _tiled_rows("tile32", (40, 80))
         + [_row("tile32", 129, 77, "randn", d=80, scale=0.05, bf=True, tag=("scale",)),
            _row("tile32", 161, 65, "one_loud_query", d=40, N=3, batch_slice=True, tag=("batch_slice",))]
         + _tiled_rows("tile32_2blocks", (40,))
         + _pp_rows("attention40pp_32q") + _pp_rows("attention40pp_64q")
         + [_row("attention40pp_32q", 257, 192, "randn", N=3, batch_slice=True, scale=0.3, tag=("batch_slice", "scale"))]
         + _kvres_rows()
         + [_row("kv_resident", 95, 77, "randn", d=40, N=3, heads=6, batch_slice=True, scale=0.11, tag=("batch_slice", "scale"))])


def row_id(r):
    return (f"{r['variant']}{'' if r['expect'] == r['variant'] else '->' + r['expect']} N={r['N']} heads={r['heads']} Sq={r['Sq']} Skv={r['Skv']} d={r['d']} "
            f"{'bf16' if r['bf'] else 'fp16'} {r['kind']} seed={r['seed']}{'' if r['scale'] is None else ' scale=' + str(r['scale'])}"
            f"{' kvres=' + str(r['kvres']) if r['kvres'] != ATTN_KERNELS[r['variant']][2] else ''}{' buf[1:4]' if r['batch_slice'] else ''}")


def validate(r):
    """a row goes to the kernel it names - by the dispatcher's rules as nm.attn_route restates them, under the knobs its child runs with - for
    the reason it is in the table for, with that kernel's geometry, and stays inside the size limits"""
    ex, d, Sq, Skv = r["expect"], r["d"], r["Sq"], r["Skv"]
    assert Sq <= 600 and Skv <= 320 and r["heads"] <= 12, row_id(r)
    assert r["N"] <= 3 or (r["heads"] == 1 and r["variant"] == "kv_resident" and (r["kvres"] == 1 or "qper" in r["tag"])), row_id(r)
    assert d in ALL_WIDTHS and (Skv >= 2 or r["kind"] == "randn") and (not r["batch_slice"] or r["N"] == 3), row_id(r)
    shape = (r["N"], r["heads"], Sq, Skv, d)
    route = nm.attn_route(*shape, row_knobs(r))
    assert route["kernel"] == ATTN_KERNEL_ID[ex], (row_id(r), route)
    g = GEOMETRY[ex]        # (kernel id 1 runs 32 queries per wave at the widths that have no 16-query form: GEOMETRY states the 16-query one)
    assert g["B"] is None or (ex == "generic" and route["q_per_wave"] == 32) or (route["q_per_wg"], route["q_per_wave"]) == (g["B"], g["w"]), (row_id(r), route)
    if r["variant"] == "kv_resident" and ex != "kv_resident":
        # an edge row of the K/V-resident rule: a shape it never takes (key or query count), or one it takes only when forced and the row asks for 1
        forced = nm.attn_route(*shape, row_knobs(r, kvres=2))["kernel"] == ATTN_KERNEL_ID["kv_resident"]
        assert d in ATTN_KERNELS["kv_resident"][1] and (r["kvres"] == 1 or not forced), row_id(r)
    if r["variant"].startswith("attention40pp") and ex == "tile32_2blocks":
        # a fallback row: only the key count keeps it off the ping-pong kernel
        assert nm.attn_route(r["N"], r["heads"], Sq, 128, d, row_knobs(r))["kernel"] == ATTN_KERNEL_ID[r["variant"]], row_id(r)
    if ex in ("generic", "generic_32q", "tile32") and r["variant"] == ex:
        assert d in ATTN_KERNELS[ex][1] or "width" in r["tag"], row_id(r)
    if "qper" in r["tag"]:
        qper, strips = kvres_strips(r["N"], r["heads"], Sq)
        assert qper > 32 and 0 < Sq - (strips - 1) * qper < qper and (Sq - (strips - 1) * qper) % 32 != 0, (row_id(r), qper, strips)


def row_classes(r):
    """the classes a row meets, for the variant whose kernel it runs"""
    if r["expect"] != r["variant"]:
        return set(r["tag"])
    g = GEOMETRY[r["variant"]]
    out = set(r["tag"]) | {r["kind"], "bf16" if r["bf"] else "fp16"}
    Sq, Skv = r["Sq"], r["Skv"]
    if g["keys"] == "kvres":
        out |= {f"Skv={Skv}", f"Sq={Sq}", f"heads={r['heads']}", f"d={r['d']}"}
        return out
    B, w = g["B"], g["w"]
    out |= {f"Skv={Skv}"}
    out |= {name for name, val in (("Sq=1", 1), ("Sq=B-1", B - 1), ("Sq=B+1", B + 1), ("Sq=B+w+1", B + w + 1)) if Sq == val}
    if g["two"]:                        # the last wave with a query in range: first 32-query block partly in range, second wholly out
        w0 = (Sq - 1) // 64 * 64
        if 0 < Sq - w0 < 32:
            out.add("2nd block out")
    if "width" in r["tag"]:
        out.add(f"d={r['d']}:{'bf16' if r['bf'] else 'fp16'}")
    return out


def _required(variant):
    g = GEOMETRY[variant]
    need = set(KINDS) | {"fp16", "bf16"}
    if g["keys"] == "kvres":
        need |= {f"Skv={k}" for k in KVRES_KEYS} | {f"Sq={s}" for s in KVRES_QUERIES} | {f"heads={h}" for h in KVRES_HEADS} | {"d=40", "d=80", "qper"}
        need |= {"edge_Skv97", "edge_Sq63", "edge_groups12_d40", "edge_groups11_d40", "edge_groups64_d80", "edge_groups63_d80"}
        return need
    need |= {"Sq=1", "Sq=B-1", "Sq=B+1", "Sq=B+w+1"} | ({"2nd block out"} if g["two"] else set())
    need |= {f"Skv={k}" for k in (TILED_KEYS if g["keys"] == "tiled" else PP_KEYS)}
    if g["keys"] == "pp":
        need |= {"fallback_k127", "fallback_k64"}
    if variant == "generic":
        need |= {f"d={d}:{t}" for d in ALL_WIDTHS for t in ("fp16", "bf16")}
    if variant == "generic_32q":
        need |= {f"d={d}:{t}" for d in (40, 48, 80) for t in ("fp16", "bf16")}
    return need


REQUIRED = {v: _required(v) for v in ATTN_KERNELS}
ANYWHERE = {"scale", "batch_slice"}                      # met by at least one row of the table


def coverage():
    """(printable matrix: variant -> class -> number of rows, list of (variant, class) pairs no row meets)"""
    met = {v: {} for v in ATTN_KERNELS}
    for r in TABLE:
        for c in row_classes(r):
            met[r["variant"]][c] = met[r["variant"]].get(c, 0) + 1
    lines, missing = [], []
    for v in ATTN_KERNELS:
        n = sum(r["variant"] == v for r in TABLE)
        lines.append(f"{v} ({n} rows): " + ", ".join(f"{c} x{met[v].get(c, 0)}" for c in sorted(REQUIRED[v])))
        missing += [(v, c) for c in sorted(REQUIRED[v]) if not met[v].get(c)]
    missing += [("anywhere", c) for c in sorted(ANYWHERE) if not any(c in r["tag"] for r in TABLE)]
    return "\n".join(lines), missing


for _r in TABLE:
    validate(_r)
_matrix, _missing = coverage()
assert not _missing, f"test_attention_gpu.TABLE leaves (variant, class) pairs unmet: {_missing}\n{_matrix}"
assert len({row_id(r) for r in TABLE}) == len(TABLE)
assert set(GEOMETRY) == set(ATTN_KERNELS) == set(ATTN_KERNEL_ID)


# ----------------------------------------------------------------------------------------------------------------
# the child: python -m tests.numerics --attn-child IN OUT views
# ----------------------------------------------------------------------------------------------------------------
def attention_views_child(argv):
    """every row of IN: the dense launch, then the two launches through poisoned views into guarded outputs.  The whole buffers and the
    (offset, size, stride) recipes of the views travel in the file; the child judges nothing."""
    from edgestyle_amd import ops, lib
    src, dst = argv[0], argv[1]
    rows = torch.load(src, weights_only=True)
    L = lib.load()
    first = L.es_attention_set_kvres(0)
    outs = {}
    try:
        for name, r in rows.items():
            dt = torch.bfloat16 if r["bf"] else torch.float16
            L.es_attention_set_kvres(int(r["kvres"]))
            N, Sq, C = r["q"].shape
            q, k, v = (r[t].to(DEV) for t in "qkv")
            assert q.dtype == dt and q.is_contiguous()
            outs[name + " dense"] = ops.attention(q, k, v, r["heads"], r["scale"]).cpu()
            ids = [L.es_attention_last_kernel()]
            for poison in ("nan", "huge"):
                buf = r["buf_" + poison].to(DEV)
                qv, kv, vv = (nm.view_from(buf, r["recipe_" + t]) for t in "qkv")
                out, _ = nm.attn_out_guarded(N, Sq, C, dt, device=DEV)
                y = ops.attention(qv, kv, vv, r["heads"], r["scale"], out=out)
                assert y.data_ptr() == out.data_ptr()
                ids.append(L.es_attention_last_kernel())
                outs[name + " out_" + poison] = out._base.cpu()
            outs[name + " #kernel"] = torch.tensor(ids)
        torch.cuda.synchronize()
    finally:
        L.es_attention_set_kvres(first)
    torch.save(outs, dst)


def _inputs(r):
    dtype = torch.bfloat16 if r["bf"] else torch.float16
    return nm.attn_inputs(r["kind"], r["N"], r["heads"], r["Sq"], r["Skv"], r["d"], dtype, r["seed"]), dtype


def run_variant(variant, tmp_path):
    """one child for every row of the variant; returns (failures, records, seconds in all, seconds of CPU baselines)"""
    t_start = time.time()
    rows = [r for r in TABLE if r["variant"] == variant]
    payload, kept = {}, {}
    for r in rows:
        (q, k, v), dtype = _inputs(r)
        p = dict(heads=r["heads"], scale=r["scale"], kvres=r["kvres"], bf=r["bf"], q=q.to(dtype), k=k.to(dtype), v=v.to(dtype))
        for poison in ("nan", "huge"):
            qv, kv, vv, _ = nm.attn_views(q, k, v, r["heads"], dtype, poison, batch_slice=r["batch_slice"])
            p["buf_" + poison] = qv._base
            for t, view in zip("qkv", (qv, kv, vv)):
                p["recipe_" + t] = nm.view_recipe(view)             # the same for both poisons
        payload[row_id(r)] = p
        kept[row_id(r)] = (q, k, v, dtype)
    src, dst = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
    torch.save(payload, src)
    env = ATTN_KERNELS[variant][0]
    res = subprocess.run([sys.executable, "-m", "tests.numerics", "--attn-child", src, dst, "views"], cwd=ROOT,
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    tail = res.stdout[-2000:] + res.stderr[-3000:]
    if res.returncode in (134, 139, 124, 137, -6, -11, -9) or "illegal memory access" in tail or "HIP error" in tail:
        # the child died on the GPU: nothing more is started on it in this session
        pytest.exit(f"attention child ({variant}) ended with status {res.returncode}:\n" + tail, returncode=3)
    assert res.returncode == 0, tail
    outs = torch.load(dst, weights_only=True)
    fails, records, t_cpu = [], [], 0.0
    for r in rows:
        name = row_id(r)
        q, k, v, dtype = kept[name]
        N, Sq, C = q.shape
        ids = [int(i) for i in outs[name + " #kernel"]]
        want = ATTN_KERNEL_ID[r["expect"]]
        if ids != [want] * 3:
            fails.append(f"{name}: kernels {ids} ran, {want} ({r['expect']}) was meant")
        dense = outs[name + " dense"]
        view0, check = nm.attn_out_guarded(N, Sq, C, dtype)
        recipe = nm.view_recipe(view0)
        same, guards = True, True
        for poison in ("nan", "huge"):
            buf = outs[name + " out_" + poison]
            try:
                check(buf)
            except AssertionError as e:
                guards = False
                fails.append(f"{name}: {poison}-poisoned views: {e}")
            y = nm.view_from(buf, recipe)
            if not torch.equal(y.contiguous().view(torch.int16), dense.view(torch.int16)):
                same = False
                diff = (y.float() - dense.float()).abs()
                n_diff = int((y.contiguous().view(torch.int16) != dense.view(torch.int16)).sum())
                fails.append(f"{name}: the output through {poison}-poisoned views differs from the dense launch's in {n_diff} elements "
                             f"(max |difference| {float(torch.nan_to_num(diff, nan=float('inf')).max()):.3e})")
        t0 = time.time()
        rec = dict(case=name, kernel=None, base_alg=None, base_ref=None, same=same, guards=guards, ids=ids)
        if r["Skv"] == 1:               # the softmax of one key is exactly 1: the output IS v[:, 0], whatever q and the scale are
            want_y = v.to(dtype)[:, :1].expand(N, Sq, C).contiguous()
            exact = torch.equal(dense.view(torch.int16), want_y.view(torch.int16))
            print(f"numerics: attention {name}: one key, output {'==' if exact else '!='} v[:, 0] bit for bit", flush=True)
            if not exact:
                fails.append(f"{name}: one key, but the output is not v[:, 0] bit for bit")
            rec.update(kernel=0.0 if exact else float("inf"))
        else:
            ref = nm.attn_ref64(q, k, v, r["heads"], r["scale"])
            assert float(ref.abs().max()) < 3.0e4
            e_ref = nm.row_err(nm.attn_base_ref(q, k, v, r["heads"], dtype, r["scale"]), ref)
            e_alg = nm.attn_design_err(q, k, v, r["heads"], dtype, ref, r["scale"], rowsum="rounded" if nm.attn_ones(r["d"]) else "fp32")
            t_cpu += time.time() - t0
            before = len(T.RECORD) if T.RECORD is not None else None
            judge(fails, f"attention {name}", dense, ref, e_alg, e_ref, dtype)
            rec.update(kernel=nm.row_err(dense, ref), base_alg=e_alg, base_ref=e_ref)
            if before is not None:
                del T.RECORD[before:]   # the report keeps this file's rows in a table of its own
        records.append(rec)
    return fails, records, time.time() - t_start, t_cpu


@pytest.mark.parametrize("variant", list(ATTN_KERNELS))
def test_attention_ragged_lengths_and_poisoned_views(variant, tmp_path):
    """Every row of TABLE for one kernel variant (see the module's docstring): kernel id, three launches equal bit for bit, guards intact,
    both bars against fp64, finite; one key returns v[:, 0]."""
    fails, records, secs, cpu = run_variant(variant, tmp_path)
    print(f"test_attention_gpu: {variant}: {len(records)} rows in {secs:.1f} s, of which CPU baselines {cpu:.2f} s", flush=True)
    done(fails)


def test_attention_table_covers_every_class():
    """the table's own bookkeeping, printed: every variant meets every class it is eligible for"""
    matrix, missing = coverage()
    print(f"test_attention_gpu: {len(TABLE)} rows\n{matrix}")
    assert not missing


# (N, heads, Sq, Skv, d), bf16, the kernel id under default knobs: the smallest shapes across the 512-block and 256-workgroup thresholds (kernel 6
# is reachable through ES_ATTN_PP=2 alone: the children above)
ROUTE_ROWS = [((1, 1, 17, 31, 8), False, 1), ((2, 8, 4096, 100, 80), False, 2), ((2, 8, 4096, 100, 40), False, 3), ((4, 8, 4096, 100, 40), False, 4),
              ((2, 8, 4096, 128, 40), False, 5), ((2, 8, 4096, 128, 40), True, 5), ((12, 8, 64, 77, 40), False, 7)]


def test_attention_route_is_the_launch():
    """In this process, under its own knobs: what es_attention_route answers for a shape is what es_attention then launches
    (es_attention_last_kernel is written by the launcher from its template arguments, the route is asked BEFORE the launch), the id is the one
    the rules give under default knobs, and the output meets the required-tier bar against fp64."""
    from edgestyle_amd import ops, lib
    L = lib.load()
    own = lib.AttnKnobs()
    L.es_attention_knobs(own)
    own = {name: getattr(own, name) for name in nm.ATTN_KNOBS}
    if own != nm.ATTN_KNOBS:
        print(f"test_attention_gpu: this process runs with knobs {own}, not the defaults: the literal kernel ids are not asserted")
    fails = []
    for shape, bf, want in ROUTE_ROWS:
        N, heads, Sq, Skv, d = shape
        dtype = torch.bfloat16 if bf else torch.float16
        name = f"route N={N} heads={heads} Sq={Sq} Skv={Skv} d={d} {'bf16' if bf else 'fp16'}"
        route = lib.attention_route(*shape, dtype=lib.ES_BF16 if bf else lib.ES_F16)
        assert route == nm.attn_route(*shape, own), (name, route)
        assert own != nm.ATTN_KNOBS or route["kernel"] == want, (name, route)
        q, k, v = nm.attn_inputs("randn", N, heads, Sq, Skv, d, dtype, seed=11 * Sq + Skv + d)
        y = ops.attention(q.to(dtype).to(DEV), k.to(dtype).to(DEV), v.to(dtype).to(DEV), heads).cpu()
        ran = L.es_attention_last_kernel()
        if ran != route["kernel"]:
            fails.append(f"{name}: kernel {ran} ran, the route said {route['kernel']}")
        ref = nm.attn_ref64(q, k, v, heads)
        e_ref = nm.row_err(nm.attn_base_ref(q, k, v, heads, dtype), ref)
        e_alg = nm.attn_design_err(q, k, v, heads, dtype, ref, rowsum="rounded" if nm.attn_ones(d) else "fp32")
        judge(fails, f"attention {name}", y, ref, e_alg, e_ref, dtype)
    done(fails)


def report_rows():
    """python -m tests.numerics --report --only attention: run every variant without asserting, return (records, seconds, CPU seconds)"""
    import pathlib
    import tempfile
    rows, secs, cpu = [], {}, 0.0
    for variant in ATTN_KERNELS:
        with tempfile.TemporaryDirectory() as t:
            fails, records, s, c = run_variant(variant, pathlib.Path(t))
        for f in fails:
            print("MISSED:", f)
        rows += records
        secs[variant] = s
        cpu += c
    return rows, secs, cpu
