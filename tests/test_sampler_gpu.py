"""The sampler step (es_cfg_unipc_step, es_cfg_ddim_step with es_incr) over whole trajectories against the coefficient table applied
in fp64 (tests/numerics.py, the sampler section), the step-index clamp, and the boundary kernels of csrc/elementwise.hip
(timestep_embedding, nchw_to_nhwc, nhwc_to_nchw, add, vae_sample, gather_row) against fp64 at their edges.

Bars: the fp32 latents after EVERY step within MARGIN x the error of the same recombination run in fp32 on the CPU (base_alg, same table,
same eps), finite; bit for bit model_in == latents.to(dtype) in both CFG halves, zero pad channels, es_latents_to_input reproduces
model_in; the UniPC history buffers within the same bar."""
import pytest
import torch

from tests import numerics as nm
from tests import test_numerics_gpu as T
from tests.test_numerics_gpu import done

pytestmark = pytest.mark.gpu

DEV = "cuda"
L = 4
RECORD = []                     # one dict per judged trajectory (python -m tests.numerics --report --only sampler)

# kind, steps, cfg, dtype, Lstride, B, (H, W), spacing, solver order.  5 x 7: 140 B values - less than one workgroup (B = 1) or one full
# workgroup and a tail (B = 3); 97 x 97 at B = 3: 112 908 values - 441 workgroups and a tail of 12, enough elements for "1 in 10^4".
TRAJECTORIES = [
    ("unipc", 1, True, "f", 8, 1, (5, 7), "leading", 2), ("unipc", 2, False, "b", 4, 3, (5, 7), "leading", 2),
    ("unipc", 3, True, "b", 8, 3, (97, 97), "leading", 2), ("unipc", 10, False, "f", 4, 1, (97, 97), "leading", 2),
    ("unipc", 10, True, "f", 8, 3, (97, 97), "leading", 2), ("unipc", 2, True, "f", 4, 3, (97, 97), "linspace", 2),
    ("unipc", 3, False, "f", 8, 1, (5, 7), "linspace", 1), ("unipc", 1, False, "b", 4, 3, (97, 97), "leading", 1),
    ("ddim", 1, False, "f", 4, 3, (5, 7), "leading", 1), ("ddim", 2, True, "b", 8, 1, (5, 7), "leading", 1),
    ("ddim", 10, True, "f", 8, 3, (97, 97), "leading", 1), ("ddim", 3, False, "b", 4, 1, (97, 97), "leading", 1),
    ("ddim", 10, False, "b", 8, 3, (5, 7), "leading", 1), ("ddim", 2, True, "f", 4, 3, (97, 97), "leading", 1),
]
for _kind in ("unipc", "ddim"):
    _rows = [r for r in TRAJECTORIES if r[0] == _kind]
    assert {r[1] for r in _rows} == {1, 2, 3, 10} and {r[2] for r in _rows} == {True, False} and {r[3] for r in _rows} == {"f", "b"}
    assert {r[4] for r in _rows} == {4, 8} and {r[5] for r in _rows} == {1, 3} and {r[6] for r in _rows} == {(5, 7), (97, 97)}
    assert any(r[5] == 3 and r[6] == (97, 97) and r[2] for r in _rows)


def _tid(r):
    return f"{r[0]}-T{r[1]}-{'cfg' if r[2] else 'nocfg'}-{'fp16' if r[3] == 'f' else 'bf16'}-Ls{r[4]}-B{r[5]}-{r[6][0]}x{r[6][1]}-{r[7]}-o{r[8]}"


def _table(kind, steps, spacing, order):
    from edgestyle_amd.schedulers import DDIMScheduler, UniPCMultistepScheduler
    s = DDIMScheduler() if kind == "ddim" else UniPCMultistepScheduler(solver_order=order, timestep_spacing=spacing)
    s.set_timesteps(steps)
    return s.coef_table()


def padded_table(table, pad=16):
    """the table cut from the middle of a larger NaN-filled device allocation: a missing clamp reads NaN inside the allocation"""
    rows, width = table.shape
    big = torch.full(((rows + 2 * pad) * width,), float("nan"), dtype=torch.float32, device=DEV)
    view = big[pad * width:(pad + rows) * width].view(rows, width)
    view.copy_(table)
    return big, view


def _step(ops, kind, noise, lat, hist, model_in, coef, idx, gs, cfg):
    if kind == "unipc":
        ops.cfg_unipc_step(noise, lat, hist[0], hist[1], hist[2], model_in, coef, idx, gs, cfg)
    else:
        ops.cfg_ddim_step(noise, lat, model_in, coef, idx, gs, cfg)


def run_trajectory(r):
    from edgestyle_amd import ops
    kind, steps, cfg, dt, Ls, B, (H, W), spacing, order = r
    dtype = torch.float16 if dt == "f" else torch.bfloat16
    name, gs, fails = "sampler " + _tid(r), 7.5, []
    table = _table(kind, steps, spacing, order)
    assert table.shape == (steps, 12 if kind == "unipc" else 4)
    seed = steps * 100 + H + B
    eps = nm.sampler_eps(steps, ((2 * B) if cfg else B, H, W, L), dtype, seed)
    x0 = torch.randn(B, H, W, L, generator=torch.Generator().manual_seed(seed)).float()
    t64 = nm.run_trajectory(kind, table, eps, x0, B, gs, cfg, torch.float64)
    t32 = nm.run_trajectory(kind, table, eps, x0, B, gs, cfg, torch.float32)
    _big, coef = padded_table(table)
    lat = x0.to(DEV).contiguous()
    hist = [torch.zeros_like(lat) for _ in range(3)]
    model_in = torch.full(((2 * B) if cfg else B, H, W, Ls), float("nan"), dtype=dtype, device=DEV)
    ops.latents_to_input(lat, model_in, cfg)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = dict(kernel=0.0, base_alg=0.0, ratio=0.0)
    names = ("latents", "last_sample", "m0", "m1")
    for i in range(steps):
        _step(ops, kind, eps[i].to(DEV, dtype), lat, hist, model_in, coef, idx, gs, cfg)
        ops.incr(idx)
        torch.cuda.synchronize()
        assert int(idx.item()) == i + 1
        got = [lat] + (hist if kind == "unipc" else [])
        for j, g in enumerate(got):
            ref, alg = t64[i][j], t32[i][j]
            if float(ref.abs().max()) == 0.0:           # m1 of the first step: zeros in, zeros out
                if float(g.abs().max()) != 0.0:
                    fails.append(f"{name} step {i}: {names[j]} must still be zero")
                continue
            e, e_alg = nm.traj_err(g, ref), nm.traj_err(alg, ref)
            if j == 0 and e / max(e_alg, 1e-30) >= worst["ratio"]:
                worst = dict(kernel=e, base_alg=e_alg, ratio=e / max(e_alg, 1e-30), step=i)
            if not bool(torch.isfinite(g).all()):
                fails.append(f"{name} step {i}: {names[j]} not finite")
            if not ((e_alg > 0 or j > 0) and e <= nm.MARGIN * e_alg) and T.RECORD is None:      # (step 0: last_sample is the start, exactly)
                fails.append(f"{name} step {i}: {names[j]} {e:.3e} > {nm.MARGIN} x base_alg {e_alg:.3e}")
        want = lat.to(dtype)
        halves = [model_in[:B], model_in[B:]] if cfg else [model_in]
        for h, half in enumerate(halves):
            n = int((half[..., :L] != want).sum())
            if n:
                fails.append(f"{name} step {i}: model_in half {h} differs from latents.to(dtype) in {n} of {want.numel()} elements")
            if Ls > L and not bool((half[..., L:] == 0).all()):
                fails.append(f"{name} step {i}: pad channels of half {h} are not zero")
        again = torch.full_like(model_in, float("nan"))
        ops.latents_to_input(lat, again, cfg)
        if not torch.equal(again, model_in):
            fails.append(f"{name} step {i}: es_latents_to_input does not reproduce model_in")
    print(f"numerics: {name}: latents, worst step {worst.get('step')}: kernel {worst['kernel']:.3e}  base_alg {worst['base_alg']:.3e}  "
          f"kernel/alg {worst['ratio']:.2f}", flush=True)
    RECORD.append(dict(case=name, **worst))
    return fails


@pytest.mark.parametrize("r", TRAJECTORIES, ids=_tid)
def test_sampler_trajectory(r):
    done(run_trajectory(r))


@pytest.mark.parametrize("kind", ["unipc", "ddim"])
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_step_index_is_clamped(kind, dtype):
    """step indices -3 and nsteps + 5 give the results of rows 0 and nsteps - 1, bit for bit.  The coefficient table is cut from the
    middle of a larger NaN-filled allocation (16 rows either side): a missing clamp reads NaN inside that allocation and nothing else."""
    from edgestyle_amd import ops
    steps, B, H, W, Ls, cfg, gs = 6, 3, 5, 7, 8, True, 5.0
    _big, coef = padded_table(_table(kind, steps, "leading", 2))
    g = torch.Generator().manual_seed(11)
    noise = torch.randn(2 * B, H, W, L, generator=g).to(DEV, dtype)
    start = [torch.randn(B, H, W, L, generator=g).to(DEV) for _ in range(4)]          # latents and a history that is not zero

    def run(i):
        lat, *hist = [t.clone() for t in start]
        model_in = torch.zeros(2 * B, H, W, Ls, dtype=dtype, device=DEV)
        _step(ops, kind, noise, lat, hist, model_in, coef, torch.tensor([i], dtype=torch.int32, device=DEV), gs, cfg)
        torch.cuda.synchronize()
        return [lat, model_in] + hist
    for outside, inside in ((-3, 0), (steps + 5, steps - 1)):
        a, b = run(outside), run(inside)
        assert all(bool(torch.isfinite(t.float()).all()) for t in a), f"index {outside}: the table was read outside its rows"
        assert all(torch.equal(x, y) for x, y in zip(a, b)), f"index {outside} does not give row {inside}"
    assert not torch.equal(run(0)[0], run(steps - 1)[0])


def test_gather_row_is_clamped():
    from edgestyle_amd import ops
    rows, width = 5, 300                    # 300 values: two workgroups, the second one partial
    table = torch.randn(rows, width, generator=torch.Generator().manual_seed(2))
    _big, view = padded_table(table)
    for i, want in ((-3, 0), (0, 0), (2, 2), (rows - 1, rows - 1), (rows + 5, rows - 1)):
        big_out = torch.full((width + 64,), float("nan"), device=DEV)
        out = big_out[32:32 + width]
        ops.gather_row(view, torch.tensor([i], dtype=torch.int32, device=DEV), out)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), table[want]), (i, want)
        assert bool(torch.isnan(big_out[:32]).all()) and bool(torch.isnan(big_out[32 + width:]).all())


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_timestep_embedding_against_the_fp64_sinusoid(dtype):
    """t in {0, 1, 500.5, 999}, dim 320: the number of elements that differ from the correctly rounded fp64 sinusoid is within
    misrounded_bar of torch's own fp32 cos / sin of the same arguments (both round t * f in fp32: at t = 999 that alone moves the
    argument by 6e-5)"""
    from edgestyle_amd import ops
    t = torch.tensor([0.0, 1.0, 500.5, 999.0])
    ref = nm.sinusoid64(t, 320)
    y = ops.timestep_embedding(t.to(DEV), 320, dtype).float().cpu()
    n_kernel = nm.misrounded(y, ref, dtype, count=True)
    n_torch = nm.misrounded(nm.sinusoid32(t, 320, dtype), ref, dtype, count=True)
    bar = nm.misrounded_bar([n_torch])
    print(f"numerics: timestep_embedding {T._name(dtype)}: misrounded kernel {n_kernel}  torch fp32 {n_torch}  bar {bar} of {ref.numel()}; "
          f"max abs err {float((y.double() - ref).abs().max()):.3e}")
    assert y.shape == (4, 320) and bool(torch.isfinite(y).all())
    assert torch.equal(y[0], torch.cat([torch.ones(160), torch.zeros(160)]))         # t = 0: cos 0 | sin 0, exactly
    assert n_kernel <= bar, (n_kernel, n_torch, bar)


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_layout_conversions_on_non_square_maps(dtype):
    from edgestyle_amd import ops
    g = torch.Generator().manual_seed(3)
    N, C, H, W = 3, 3, 5, 7
    x = 2.0 * torch.randn(N, C, H, W, generator=g)
    for cpad in (None, 8):
        y = ops.nchw_to_nhwc(x.to(DEV), dtype, cpad=cpad).cpu()
        assert y.shape == (N, H, W, cpad or C) and y.dtype == dtype
        assert torch.equal(y[..., :C], x.permute(0, 2, 3, 1).to(dtype))               # one rounding to nearest even, bit for bit
        assert cpad is None or bool((y[..., C:] == 0).all())
    src = torch.full((N, H, W, 8), float("nan")).to(dtype)                            # Cstride 8 > C 3: the NaN channels must never be read
    src[..., :C] = (2.0 * torch.randn(N, H, W, C, generator=g)).to(dtype)
    for Cs, inp in ((8, src), (C, src[..., :C].contiguous())):
        for scale, shift, clamp in ((1.0, 0.0, False), (0.5, 0.5, True), (0.37, -1.25, False), (3.0, 0.25, True)):
            z = ops.nhwc_to_nchw(inp.to(DEV), channels=C, scale=scale, shift=shift, clamp01=clamp).cpu()
            assert z.shape == (N, C, H, W) and z.dtype == torch.float32
            s32, h32 = float(torch.tensor(scale, dtype=torch.float32)), float(torch.tensor(shift, dtype=torch.float32))
            v = src[..., :C].double().permute(0, 3, 1, 2)
            ref = v * s32 + h32
            tol = 2.0 ** -23 * torch.maximum((v * s32).abs(), ref.abs()) + 1e-45      # one fp32 rounding of the product, one of the sum
            if clamp:
                ref = ref.clamp(0.0, 1.0)
            assert bool(((z.double() - ref).abs() <= tol).all()), (Cs, scale, shift, clamp, float((z.double() - ref).abs().max()))
            if clamp:
                assert float(z.min()) >= 0.0 and float(z.max()) <= 1.0 and float(z.min()) == 0.0 and float(z.max()) == 1.0


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("n", [8, 8 * (2048 * 256 + 3)])
def test_add_is_exact(n, dtype):
    """n = 8: one vector; n = 8 (2048 256 + 3): more vectors than a grid of 2048 workgroups holds threads - the grid-stride loop and its
    tail.  Exact against the correctly rounded fp64 sum; the words around the output stay untouched."""
    from edgestyle_amd import ops
    g = torch.Generator().manual_seed(n % 1000)
    a, b = torch.randn(n, generator=g).to(dtype), torch.randn(n, generator=g).to(dtype)
    big = torch.full((n + 128,), float("nan"), dtype=dtype, device=DEV)
    out = big[64:64 + n]
    y = ops.add(a.to(DEV), b.to(DEV), out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    want = nm.round64(a.double() + b.double(), dtype)
    assert torch.equal(out.float().cpu(), want), int((out.float().cpu() != want).sum())
    assert bool(torch.isnan(big[:64]).all()) and bool(torch.isnan(big[64 + n:]).all())


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_vae_sample_at_and_beyond_the_clamps(dtype):
    """logvar at and beyond both clamps (-40, -30, 20, 25), Lpad 8 > L 4, a 5 x 7 map: finite wherever the rounded fp64 reference is,
    row_err (rows = pixels) <= MARGIN x the textbook sequence with every op rounded to the storage dtype, zero pad channels"""
    from edgestyle_amd import ops
    g = torch.Generator().manual_seed(4)
    N, H, W, Lpad, scaling = 3, 5, 7, 8, 0.18215
    mom = torch.randn(N, H, W, 2 * L, generator=g)
    edge = torch.tensor([-40.0, -30.0, 20.0, 25.0, -30.5, 19.5])
    pick = torch.randint(0, len(edge), (N, H, W, L), generator=g)
    mom[..., L:] = torch.where(torch.rand(N, H, W, L, generator=g) < 0.5, edge[pick], mom[..., L:])
    mom = nm.rnd(mom, dtype)
    noise = torch.randn(N, L, H, W, generator=g)
    s32 = float(torch.tensor(scaling, dtype=torch.float32))
    ref = nm.vae_sample_ref(mom, noise, L, s32, torch.float64)
    base = nm.vae_sample_ref(mom, noise, L, s32, torch.float32, dtype)
    z = ops.vae_sample(mom.to(DEV, dtype), noise.to(DEV), L, Lpad, scaling).float().cpu()
    assert z.shape == (N, H, W, Lpad) and bool((z[..., L:] == 0).all())
    y = z[..., :L]
    assert nm.finite_where_representable(y, ref, dtype)
    ok = torch.isfinite(nm.rnd(ref, dtype)).all(dim=-1)                             # pixels the storage dtype can hold
    assert float(ok.double().mean()) > 0.5
    held = ok & torch.isfinite(base).all(dim=-1)                                   # ... and the textbook sequence's intermediates (std * noise) too
    assert float(held.double().mean()) > 0.5
    e, e_ref = nm.row_err(y[ok], ref[ok]), nm.row_err(base[held], ref[held])
    print(f"numerics: vae_sample {T._name(dtype)}: kernel {e:.3e}  base_ref {e_ref:.3e}  largest reference {float(ref.abs().max()):.3e}")
    assert e_ref > 0 and e <= nm.MARGIN * e_ref, (e, e_ref)


def report_rows():
    """python -m tests.numerics --report --only sampler: run every trajectory without asserting, return (records, seconds)"""
    import time
    del RECORD[:]
    t0 = time.time()
    for r in TRAJECTORIES:
        run_trajectory(r)
    return list(RECORD), time.time() - t0
