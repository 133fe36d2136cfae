"""Thin Python wrappers over the C ABI: torch only allocates device memory and supplies the current HIP stream.

Internal activation layout is NHWC ([N,H,W,C], dtype fp16/bf16); every wrapper launches on
`torch.cuda.current_stream()` so the calls can be captured into a hipGraph (`torch.cuda.graph`).
"""
import ctypes as C
import math
import os as _os
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import lib as L

_DT = {torch.float16: L.ES_F16, torch.bfloat16: L.ES_BF16}
LANE = 0            # scratch-buffer namespace: concurrent chains on different HIP streams must not share scratch


class lane:
    """with ops.lane(i): ... — kernels launched inside use scratch buffers (split-K workspace, GroupNorm partials)
    private to lane i, so independent chains can run concurrently on separate streams."""

    def __init__(self, i: int):
        self.i = i

    def __enter__(self):
        global LANE
        self.prev, LANE = LANE, self.i

    def __exit__(self, *a):
        global LANE
        LANE = self.prev


XCD_ORDER = -1      # tuning knob: -1 auto, 0 tile_n fastest, 1 tile_m fastest
DEEP_RING = _os.environ.get("ES_DEEP_RING", "1") == "1"     # 4-stage LDS ring for launches of <= 1 workgroup per CU
FORCE_BN = 0        # tuning knob: 0 = per-launch choice between the legal N tiles
FORCE_STAGES = 0    # tuning knob (tools/gemm_bench.py): 0 = kernel picks the LDS ring depth
FORCE_WAVES = 0     # tuning knob: 0 = planner picks 4 or 8 waves per 128-pixel workgroup
EIGHT_WAVES = _os.environ.get("ES_EIGHT_WAVES", "1") == "1"
SMALL_TILE = _os.environ.get("ES_SMALL_TILE", "1") == "1"    # 64x64 tile for tiny launches
PROFILE = None      # set to a Profiler by bench.py: every es_conv_gemm launch gets an in-kernel timing slot


class Profiler:
    """Per-launch durations as executed (also inside a hipGraph replay, where host-side events cannot look):
    each workgroup of an instrumented launch atomically mins its start / maxes its end s_memrealtime stamp
    (100 MHz constant clock) into a device slot; duration = (max end - min start) * 10 ns."""

    def __init__(self, device, capacity: int = 8192, stamps: bool = True):
        self.slots = torch.empty((capacity, 2), dtype=torch.int64, device=device)
        self.meta = []
        self.stamps = stamps        # False: only record the descriptors (launch list), no in-kernel atomics
        self.descs = []             # a copy of every es_gemm_desc launched while this profiler was active
        self.reset()

    def reset(self):
        self.slots[:, 0] = 1 << 62
        self.slots[:, 1] = 0

    def next(self, meta) -> int:
        i = len(self.meta)
        if i >= self.slots.shape[0]:
            raise L.EdgeStyleHipError("Profiler capacity exceeded")
        self.meta.append(meta)
        return self.slots[i].data_ptr() if self.stamps else 0

    def replay_gemms(self, only_ksize: int = 0):
        """Launch the recorded es_conv_gemm descriptors again on the current stream, un-instrumented (the production
        kernel: no stamp atomics).  The buffers they point at must still be alive (keep the graph that owns them).
        only_ksize = 3: only the 3x3 convolutions."""
        lib = L.load()
        for d in self.descs:
            if only_ksize and (isinstance(d, L.XsDesc) or int(d.ksize) != only_ksize):
                continue
            fn = lib.es_linear_xs if isinstance(d, L.XsDesc) else lib.es_conv_gemm
            L.check(fn(C.byref(d), _stream()), "GEMM replay")

    def results(self, first: int = 0):
        s = self.slots[first:len(self.meta)].cpu().tolist()
        return [(m, (e - b) * 1e-8) for m, (b, e) in zip(self.meta[first:], s) if e > 0]
BK = 64
BM = 128


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise L.EdgeStyleHipError(f"unsupported dtype {t.dtype}: the HIP path computes in fp16 or bf16")


# ----------------------------------------------------------------------------------------------------------------
# weight packing (host side, once at load)
# ----------------------------------------------------------------------------------------------------------------
@dataclass
class PackedWeight:
    w: torch.Tensor                 # [rows_padded, Kpad] dtype, K = (ky,kx,c) tap-major
    bias: Optional[torch.Tensor]    # [rows_padded] fp32
    cout: int                       # true GEMM N
    cin: int                        # padded input channels (multiple of 8)
    ksize: int
    bn: int
    geglu: bool = False
    ln_colsum: Optional[torch.Tensor] = None   # fp32 [rows_padded]: LayerNorm folded into this linear layer (pack_weight_ln)
    ln_eps: float = 1e-5
    ctail: int = 0                  # channels of the 1x1 tail sources appended along K (pack_weight_tail)
    korder: int = 0                 # K order of the k*k*cin main part: 0 tap-major (ky,kx,c), 1 chunk-major (c/64,ky,kx,c%64)

    @property
    def rows_padded(self):
        return self.w.shape[0]

    @property
    def kpad(self):
        return self.w.shape[1]


def choose_bn(cout: int) -> int:
    return 160 if (cout % 160 == 0 and cout % 128 != 0) else 128


# K order of the 3x3 convolutions (es_gemm_desc.korder).  Chunk-major - the nine taps of a 64-channel chunk back to back - makes
# eight of a workgroup's nine shifted reads of the same activation lines L2 hits: the level-0 batch-8 launch fetches 0.39 GB
# through the fabric instead of 2.6 GB (FETCH_SIZE, profiles/r04_korder_pmc.txt).  It is nevertheless 5-10 % SLOWER in every
# sustained A/B (profiles/r04_korder_bench.txt), even with eight of the nine activation DMAs removed altogether
# (profiles/r04_patchsim_ablation.txt), so it is OFF by default: ES_CHUNK_MAJOR=1 (read by csrc/builder.hip too) turns it on.
CHUNK_MAJOR = _os.environ.get("ES_CHUNK_MAJOR", "0") == "1"


def choose_korder(k: int, cin_padded: int) -> int:
    """es_gemm_desc.korder of a convolution's packed weights (csrc/builder.hip: the same rule)."""
    return 1 if (CHUNK_MAJOR and k == 3 and cin_padded % BK == 0) else 0


def _chunk_major(w: torch.Tensor, k: int, cin: int) -> torch.Tensor:
    """[Cout, k*k*cin] tap-major -> chunk-major."""
    cout = w.shape[0]
    return w.reshape(cout, k * k, cin // BK, BK).permute(0, 2, 1, 3).reshape(cout, k * k * cin)


def pack_weight(weight: torch.Tensor, bias: Optional[torch.Tensor], dtype, device, geglu: bool = False,
                cin_pad: Optional[int] = None, cout_pad: Optional[int] = None) -> PackedWeight:
    """weight: [Cout, Cin, k, k] (conv) or [Cout, Cin] (linear) fp32, on any device -> packed tensor on `device`.

    GEGLU (ff.net.0.proj, out = 2*inner): rows are re-ordered in blocks of 32 = [16 hidden | 16 gate] so that
    the GEMM epilogue finds hidden and gate of the same output column in adjacent MFMA fragments.
    `cout_pad` appends zero output channels (used to hand 4-channel latents on as 8-channel NHWC tensors).
    """
    if weight.dim() == 2:
        weight = weight[:, :, None, None]
    weight = weight.to(device=device, dtype=torch.float32)
    cout, cin, k, _ = weight.shape
    cp = cin_pad or ((cin + 7) // 8 * 8)
    w = weight.permute(0, 2, 3, 1)                              # [Cout, k, k, Cin]
    if cp != cin:
        w = torch.nn.functional.pad(w, (0, cp - cin))
    w = w.reshape(cout, k * k * cp)
    korder = choose_korder(k, cp)
    if korder:
        w = _chunk_major(w, k, cp)
    b = None if bias is None else bias.to(device=device, dtype=torch.float32)
    if geglu:
        inner = cout // 2
        assert inner % 16 == 0
        idx = torch.arange(cout, device=device)
        blk, within = idx // 32, idx % 32
        src = torch.where(within < 16, blk * 16 + within, inner + blk * 16 + (within - 16))
        w = w[src]
        if b is not None:
            b = b[src]
    cout_eff = cout_pad or cout
    bn = 128 if geglu else choose_bn(cout_eff)
    rows = (cout_eff + bn - 1) // bn * bn
    ktrue = w.shape[1]
    kpad = (ktrue + BK - 1) // BK * BK
    wp = torch.zeros(rows, kpad, dtype=dtype, device=device)
    wp[:cout, :ktrue] = w.to(dtype)
    bp = None
    if b is not None:
        bp = torch.zeros(rows, dtype=torch.float32, device=device)
        bp[:cout] = b
    return PackedWeight(wp, bp, cout_eff, cp, k, bn, geglu, korder=korder)


def pack_weight_tail(weight: torch.Tensor, tail_weight: torch.Tensor, bias: Optional[torch.Tensor], dtype, device) -> PackedWeight:
    """conv (weight [Cout,Cin,k,k]) and a 1x1 conv over OTHER tensors of the output's size (tail_weight [Cout,Ct] or
    [Cout,Ct,1,1]) as one GEMM: K = (ky,kx,c) taps of the conv, then the tail channels (es_gemm_desc.t1/t2).
    ResnetBlock2D: conv2(h) + conv_shortcut(x); `bias` is the SUM of the two biases.  64-aligned channels only."""
    weight = weight.to(device=device, dtype=torch.float32)
    tw = tail_weight.to(device=device, dtype=torch.float32).reshape(tail_weight.shape[0], -1)
    cout, cin, k, _ = weight.shape
    if cin % BK or tw.shape[1] % BK or tw.shape[0] != cout:
        raise L.EdgeStyleHipError("pack_weight_tail: conv and tail channels must be multiples of 64, equal Cout")
    korder = choose_korder(k, cin)
    wm = weight.permute(0, 2, 3, 1).reshape(cout, k * k * cin)
    w = torch.cat([_chunk_major(wm, k, cin) if korder else wm, tw], 1)
    bn = choose_bn(cout)
    rows = (cout + bn - 1) // bn * bn
    wp = torch.zeros(rows, w.shape[1], dtype=dtype, device=device)
    wp[:cout] = w.to(dtype)
    bp = None
    if bias is not None:
        bp = torch.zeros(rows, dtype=torch.float32, device=device)
        bp[:cout] = bias.to(device=device, dtype=torch.float32)
    return PackedWeight(wp, bp, cout, cin, k, bn, False, ctail=tw.shape[1], korder=korder)


def pack_weight_ln(weight: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                   eps: float, dtype, device, geglu: bool = False) -> PackedWeight:
    """Linear(LayerNorm(x)) as ONE launch on the raw x (es_gemm_desc.ln_colsum):
        LN(x) W^T + b = rstd (x (W*gamma)^T - mean colsum(W*gamma)) + (W beta + b)
    The kernel gathers every row's mean / rstd from the activation tiles it stages anyway.  weight: [Cout, Cin]."""
    w = weight.to(device=device, dtype=torch.float32)
    if w.dim() == 4:
        w = w[:, :, 0, 0]
    g = gamma.to(device=device, dtype=torch.float32)
    b = beta.to(device=device, dtype=torch.float32)
    # the two reductions in double, rounded once (order-independent: es_load_weights computes the same values on the host)
    fb = w.double() @ b.double()
    if bias is not None:
        fb = fb + bias.to(device=device, dtype=torch.float64)
    pw = pack_weight(w * g[None, :], fb.float(), dtype, device, geglu=geglu)
    pw.ln_colsum = pw.w.double().sum(dim=1).float().contiguous()          # of the ROUNDED weights the MFMAs multiply
    pw.ln_eps = float(eps)
    return pw


# ----------------------------------------------------------------------------------------------------------------
# split-K workspace (grown outside graph capture by a warm-up pass)
# ----------------------------------------------------------------------------------------------------------------
_workspace = {}
_workspace_retired = []


def _get_workspace(nbytes: int, device) -> torch.Tensor:
    device = (device, LANE)
    ws = _workspace.get(device)
    if ws is None or ws.numel() * 4 < nbytes:
        if torch.cuda.is_current_stream_capturing():
            raise L.EdgeStyleHipError("split-K workspace too small during graph capture; run one eager warm-up first")
        if ws is not None:
            _workspace_retired.append(ws)      # graphs captured earlier still write their slabs there: never freed
        ws = torch.empty(max(nbytes // 4, 1 << 22), dtype=torch.float32, device=device[0])
        _workspace[device] = ws
    return ws


# Launch planner: the cost model, its constants and what they were fitted on live with the launch policy (csrc/launch_policy.hip).
# the 256 x 320 phase-interleaved tile (csrc/gemm_conv8p.hip)
BIG_TILE = _os.environ.get("ES_BIG_TILE", "1") == "1"
BIG_TILE_256 = _os.environ.get("ES_BIG_TILE_256", "1") != "0"     # its 256-wide form for the LayerNorm-folded / GEGLU linear layers


def plan_gemm(M: int, rows_padded: int, kpad: int, geglu: bool = False, bns=(160, 128, 64), allow_split: bool = True):
    """(bn, splitk, stages) of an es_conv_gemm launch among the tiles `bns`: the library's planner (es_plan_gemm_choice,
    csrc/launch_policy.hip), the one inside the launch policy both hosts ask (es_launch_choose).  For tools and tests; tests/numerics.py
    holds its independent restatement (plan_gemm_reference), which tests/test_load_weights_cpu.py sweeps the library against."""
    arr = (C.c_int * len(bns))(*[int(b) for b in bns])
    bn, sk, st = C.c_int(), C.c_int(), C.c_int()
    if L.load().es_plan_gemm_choice(int(M), int(rows_padded), int(kpad), int(bool(geglu)), arr, len(bns), int(bool(allow_split)),
                                    C.byref(bn), C.byref(sk), C.byref(st)) != 0:
        raise L.EdgeStyleHipError(f"plan_gemm: rows_padded {rows_padded} fits no N tile")
    stages = st.value
    if stages == 4 and not (DEEP_RING and LANE == 0):       # tool knobs: no 4-deep ring
        stages = 2
    return bn.value, sk.value, stages


def choose_launch_bn(M: int, pw: "PackedWeight") -> int:
    return plan_gemm(M, pw.rows_padded, pw.kpad, pw.geglu)[0]


def choose_splitk(M: int, rows_padded: int, bn: int, kpad: int) -> int:
    return plan_gemm(M, rows_padded, kpad, bns=(bn,))[1]


def plan_launch(M: int, pw: "PackedWeight", bn: int):
    """(splitk, stages) for a fixed N tile."""
    _, sk, st = plan_gemm(M, pw.rows_padded, pw.kpad, pw.geglu, bns=(bn,))
    return sk, st


XS_ENABLED = _os.environ.get("ES_XS", "1") == "1"      # row-stationary short-K linear kernel (csrc/linear_xs.hip)
XS_RESIDUAL = _os.environ.get("ES_XS_RESIDUAL", "1") == "1"   # ... also for the K = 320 output projections that add a residual
XS_FORCE_SLICES = 0                                    # tool knob (tools/xs_slices_bench.py): cut every launch into this many slices
XS_MIN_M = int(_os.environ.get("ES_XS_MIN_M", "8192"))   # 0: no size policy (tests exercise every shape)
_zero_bias = {}


def launch_knobs(**over) -> "L.LaunchKnobs":
    """es_launch_knobs from this module's switches and tool knobs as they stand NOW (tests and tools set the attributes)."""
    kn = dict(xs_enabled=XS_ENABLED, xs_residual=XS_RESIDUAL, xs_min_m=XS_MIN_M, big_tile=BIG_TILE, big_tile_256=BIG_TILE_256,
              small_tile=SMALL_TILE, eight_waves=EIGHT_WAVES, deep_ring=DEEP_RING and LANE == 0,
              gn_handover=(2 if GN_HANDOVER_ALL else 1) if GN_HANDOVER else 0, wide_stream={"auto": -1, "1": 1}.get(WIDE_STREAM, 0),
              gn_fold=GN_FOLD, force_bn=FORCE_BN, force_waves=FORCE_WAVES, force_stages=FORCE_STAGES, xcd_order=XCD_ORDER)
    return L.LaunchKnobs(**{k: int(v) for k, v in dict(kn, **over).items()})


def launch_query(M: int, hw: int, pw: "PackedWeight", pws=None, group_n=None, **facts) -> "L.LaunchQuery":
    """es_launch_query of a launch of `pw` (grouped: `pws`, `group_n` samples each) over M pixels, hw per sample; `facts`: whatever
    differs from a plain linear call."""
    q = L.LaunchQuery(M=M, hw=hw, w_numel=pw.w.numel(), ksize=pw.ksize, stride=1, rows_padded=pw.rows_padded, kpad=pw.kpad, cin=pw.cin,
                      ctail=pw.ctail, cout=pw.cout, geglu=pw.geglu, has_ln=pw.ln_colsum is not None, residual_dense=1, unit_scale=1, x_rep=1)
    for name, v in facts.items():
        setattr(q, name, int(v))
    if pws is not None:
        q.ngroups, q.groups_agree = len(pws), all((p.ln_colsum is None) == (pw.ln_colsum is None) for p in pws)
    if group_n is not None:
        q.n_counts = len(group_n)
        q.group_n[:] = (list(group_n) + [0] * 4)[:4]
    return q


def xs_eligible(M: int, pw: "PackedWeight", pws, group_n, hw: int) -> bool:
    """Does this plain linear launch go to es_linear_xs?"""
    return L.load().es_launch_route(C.byref(launch_query(M, hw, pw, pws, group_n)), C.byref(launch_knobs(force_bn=0))) == L.ROUTE_LINEAR_XS


def linear_xs(x: torch.Tensor, pw, M: int, out: torch.Tensor, group_rows=None, residual: Optional[torch.Tensor] = None,
              gn: Optional[dict] = None) -> torch.Tensor:
    """x: [M, K] contiguous; pw (or list of pw for a grouped launch with `group_rows` rows each) -> out [M, cstore]
    (+ residual [M, cstore]: K = 320 only).  out (and residual, with the SAME pitch: the kernel reads it with out's) may be row-pitched
    views: inner stride 1, a row pitch of whole 16-byte vectors >= cstore.  group_rows: runs of whole 256-row blocks, the last may be
    ragged.  gn = dict(part, gamma, beta, groups, nchunk, hw, eps): GroupNorm in front (es_xs_desc.gn_part; gamma / beta lists for a
    grouped launch).  The launch takes data_ptr()s, M and one pitch: whatever it would read or write differently from what the tensors
    hold is refused here, before anything is recorded or launched."""
    def bad(msg):
        return L.EdgeStyleHipError("linear_xs: " + msg)
    pws = None
    if isinstance(pw, (list, tuple)):
        pws = list(pw) if len(pw) > 1 else None
        pw = pw[0]
    cstore = pw.cout // 2 if pw.geglu else pw.cout
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise bad(f"x must be fp16 or bf16, not {x.dtype}")
    for name, t in (("out", out), ("residual", residual)):
        if t is not None and (t.dtype != x.dtype or t.device != x.device):
            raise bad(f"{name} is {t.dtype} on {t.device}, x is {x.dtype} on {x.device}")
    if M < 1 or x.dim() != 2 or tuple(x.shape) != (M, pw.kpad) or not x.is_contiguous():
        raise bad(f"x must be a contiguous [M, K] = [{M}, {pw.kpad}] (got shape {tuple(x.shape)}, strides {x.stride()})")
    if x.device.type != "meta" and x.data_ptr() % 16:
        raise bad("x must start at a multiple of 16 bytes (16-byte vector loads)")
    for name, t in (("out", out), ("residual", residual)):
        if t is None:
            continue
        if t.dim() != 2 or tuple(t.shape) != (M, cstore):
            raise bad(f"{name} must be [M, cstore] = [{M}, {cstore}], not {tuple(t.shape)}")
        if t.stride(1) != 1:
            raise bad(f"{name}: innermost stride must be 1")
    ldo = out.stride(0) if M > 1 else cstore                # (one row: its pitch is never used)
    if ldo < cstore or ldo % 8:
        raise bad(f"out: row pitch {ldo} must be a multiple of 8 elements and at least the width {cstore}")
    if residual is not None and M > 1 and residual.stride(0) != ldo:
        raise bad(f"residual: row pitch {residual.stride(0)} differs from out's {ldo} (the kernel reads it with out's)")
    for name, t in (("out", out), ("residual", residual)):
        if t is not None and t.device.type != "meta" and t.data_ptr() % 16:
            raise bad(f"{name} must start at a multiple of 16 bytes (16-byte vector accesses)")
    if pws is not None:
        if group_rows is None or len(group_rows) != len(pws) or sum(group_rows) != M or any(n < 1 for n in group_rows):
            raise bad(f"group_rows {None if group_rows is None else list(group_rows)} must hold one run of rows per weight set and sum to M = {M}")
        if any(n % 256 for n in list(group_rows)[:-1]):
            raise bad(f"group_rows {list(group_rows)}: every run but the last must be whole 256-row blocks")
    K = pw.kpad
    nslices, cps = C.c_int32(), C.c_int32()
    L.check(L.load().es_launch_xs_slices(M, K, pw.cout, int(pw.geglu), XS_FORCE_SLICES, C.byref(nslices), C.byref(cps)), "es_launch_xs_slices")
    d = L.XsDesc()
    d.x, d.out = x.data_ptr(), out.data_ptr()

    def bias_of(q):
        if q.bias is not None:
            return q.bias.data_ptr()
        key = (x.device, q.rows_padded)
        z = _zero_bias.get(key)
        if z is None:
            z = _zero_bias[key] = torch.zeros(q.rows_padded, dtype=torch.float32, device=x.device)
        return z.data_ptr()
    d.w, d.bias = pw.w.data_ptr(), bias_of(pw)
    d.M, d.K, d.Cout, d.rows_padded = M, K, pw.cout, pw.rows_padded
    d.ldo = ldo
    d.geglu, d.ln, d.ln_eps = int(pw.geglu), int(pw.ln_colsum is not None), pw.ln_eps
    d.nslices, d.chunks_per_slice, d.dtype = nslices.value, cps.value, _dt(x)
    d.residual = residual.data_ptr() if residual is not None else None
    if gn is not None:
        d.gn_part, d.gn_groups, d.gn_nchunk, d.gn_hw, d.gn_eps = gn["part"].data_ptr(), gn["groups"], gn["nchunk"], gn["hw"], gn["eps"]
        gam, bet = gn["gamma"], gn["beta"]
        if pws is not None:
            if len(gam) != len(pws) or len(bet) != len(pws):
                raise L.EdgeStyleHipError("grouped linear_xs: one GroupNorm parameter set per weight group")
            for g in range(len(pws)):
                d.gn_gamma_g[g], d.gn_beta_g[g] = gam[g].data_ptr(), bet[g].data_ptr()
        else:
            if isinstance(gam, (list, tuple)):
                gam, bet = gam[0], bet[0]
            d.gn_gamma, d.gn_beta = gam.data_ptr(), bet.data_ptr()
    if pws is not None:
        d.ngroups = len(pws)
        acc = 0
        for g, (q, n) in enumerate(zip(pws, group_rows)):
            if (q.rows_padded, q.kpad, q.cout, q.geglu) != (pw.rows_padded, pw.kpad, pw.cout, pw.geglu):
                raise L.EdgeStyleHipError("grouped linear_xs: weight geometry differs between groups")
            acc += n
            d.mt_end[g] = (acc + 127) // 128                 # (whole 256-row blocks, checked above; the last run: ceil(M / 128))
            d.w_g[g] = q.w.data_ptr()
            d.bias_g[g] = bias_of(q)
    if PROFILE is not None:
        d.prof = PROFILE.next((2.0 * M * pw.cout * K, 1, (M, pw.cout, K, 1, 1, 0),
                               dict(N=M, H=1, W=1, C1=K, C2=0, cout=pw.cout, k=1, stride=1, pad=0, upsample=False,
                                    geglu=pw.geglu, splitk=1, Hout=1, Wout=1, residual=residual is not None, temb=False, bn=0, stages=3,
                                    group_n=list(group_rows) if pws is not None else None, ctail=0, kernel="linear_xs",
                                    algorithmic_bytes=_algorithmic_bytes(x, None, pw, pws, out, residual))))
        dd = L.XsDesc()
        C.memmove(C.byref(dd), C.byref(d), C.sizeof(L.XsDesc))
        dd.prof = None
        PROFILE.descs.append(dd)
    L.check(L.load().es_linear_xs(C.byref(d), _stream()), "es_linear_xs")
    return out


# Wide residual stream (es_gemm_desc.residual_lo / out_lo): the tensors every block adds into travel as hi + lo, the low part riding
# on the tensor object as `._lo`.  "auto" (default): bf16 pipelines only - bf16 keeps 8 significant bits, and the rounding of the
# stream's sums, accumulating from block to block, was 5 dB of configs[4]'s error (profiles/r04_bf16_error_budget_2steps.txt);
# fp16 pipelines keep the single-tensor stream (11 bits; nothing measurable to gain, bandwidth to lose).  ES_WIDE_STREAM=0 | 1 forces.
WIDE_STREAM = _os.environ.get("ES_WIDE_STREAM", "auto")


# GroupNorm statistics handed over by the producing GEMM (es_gemm_desc.gn_part -> es_gn_desc.ext_chunks): the convolution whose
# output a GroupNorm normalises writes the per-(sample, 64-pixel block, group) sums from its epilogue; the GroupNorm is then one
# streaming pass (no statistics launch, no second read).  The table rides on the output tensor as `._gnp`.
# OFF by default (ES_GN_HANDOVER=1: at the 64 x 64 level, where the stand-alone GroupNorm is the two-launch form; "all": everywhere):
# built and measured in round 4, it LOSES - the epilogues' extra LDS passes and barriers cost more than the statistics launch they
# replace (batch 1: 476 vs 466 ms per image at the 64 x 64 level only, 482 everywhere; batch 8: 2623 vs 2553 ms;
# profiles/r04_gn_handover.txt) - the deeper levels' one-launch slab GroupNorm already reads its input once.
GN_HANDOVER = _os.environ.get("ES_GN_HANDOVER", "0") in ("1", "all")


def gn_handover(hw: int, c: int, groups: int) -> bool:
    """Does a GEMM whose [.., hw, c] output feeds a GroupNorm over `groups` groups hand the statistics over?  A rule of the SHAPE
    alone (grouped and per-net launches of a layer must agree): where the stand-alone GroupNorm is the two-launch form - slabs too
    large for a workgroup's registers, the 64 x 64 level - the hand-over removes its statistics launch and second read; the
    one-launch slab form of the deeper levels already reads its input once, and there the hand-over measured a net loss
    (profiles/r04_gn_handover.txt)."""
    return bool(L.load().es_launch_gn_handover(hw, c, groups, C.byref(launch_knobs())))


GN_HANDOVER_ALL = _os.environ.get("ES_GN_HANDOVER", "0") == "all"     # tool switch: also where the consumer is the slab form


def wide_stream(dtype) -> bool:
    return bool(L.load().es_launch_wide_stream(_DT.get(dtype, L.ES_F32), C.byref(launch_knobs())))


def carry_lo(dst: torch.Tensor, src: torch.Tensor, shape=None) -> torch.Tensor:
    """a view / reshape `dst` of the stream tensor `src` keeps its low part (viewed alike)"""
    lo = getattr(src, "_lo", None)
    if lo is not None:
        dst._lo = lo.reshape(dst.shape if shape is None else shape)
    return dst


def conv_gemm(x: torch.Tensor, pw: PackedWeight, *, stride: int = 1, pad: Optional[int] = None,
              upsample: bool = False, x2: Optional[torch.Tensor] = None, temb: Optional[torch.Tensor] = None,
              residual: Optional[torch.Tensor] = None, act: int = L.ACT_NONE, out_scale: float = 1.0,
              out_scale_dev: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              out_hw=None, splitk: Optional[int] = None, stages: int = 0,
              group_n: Optional[Sequence[int]] = None, tail: Optional[Sequence[torch.Tensor]] = None,
              x_rep: int = 1, wide: bool = False, out_lo: Optional[torch.Tensor] = None, gn_groups: int = 0,
              gn_part: Optional[torch.Tensor] = None):
    """x: [N,H,W,C1] (+ x2 [N,H,W,C2]); returns [N,Hout,Wout,Cout] (Cout/2 for GEGLU).

    x_rep > 1: the launch covers x_rep * N samples, sample n reading x[n % N] (es_gemm_desc.x_nmod): one sample tensor
    feeding several groups of a grouped launch without a replicated copy.

    Grouped launch: `pw` is a list of PackedWeights of identical geometry and `group_n` the number of consecutive
    samples of x each of them applies to (sum = N): one launch instead of len(pw)."""
    pws = None
    if isinstance(pw, (list, tuple)):
        pws = list(pw)
        pw = pws[0]
        if len(pws) == 1:
            pws = None
    N, H, W, C1 = x.shape
    nsrc = N
    if x_rep > 1:
        if x2 is not None or tail:
            raise L.EdgeStyleHipError("conv_gemm: x_rep needs a single source")
        N = N * x_rep
    C2 = 0 if x2 is None else x2.shape[3]
    if C1 + C2 != pw.cin:
        raise L.EdgeStyleHipError(f"conv_gemm: input channels {C1}+{C2} != packed {pw.cin}")
    tails = [t for t in (tail or ()) if t is not None]
    if sum(t.shape[3] for t in tails) != pw.ctail or len(tails) > 2:
        raise L.EdgeStyleHipError(f"conv_gemm: tail channels {[t.shape[3] for t in tails]} != packed {pw.ctail}")
    k = pw.ksize
    if pad is None:
        pad = 1 if k == 3 else 0
    Hin, Win = (H * 2, W * 2) if upsample else (H, W)
    if out_hw is None:
        Hout = (Hin + 2 * pad - k) // stride + 1
        Wout = (Win + 2 * pad - k) // stride + 1
    else:
        Hout, Wout = out_hw
    act_i = L.ACT_GEGLU if pw.geglu else act
    cstore = pw.cout // 2 if pw.geglu else pw.cout
    if out is None:
        out = torch.empty((N, Hout, Wout, cstore), dtype=x.dtype, device=x.device)
    M = N * Hout * Wout
    # the library is handed data_ptr() and the shape: a view with other strides (a channel slice, a transposed map) would be read or
    # written as if it were dense - refused here, a caller that holds such a view makes it contiguous itself
    for what, t, numel in (("x", x, None), ("x2", x2, nsrc * H * W * C2), ("residual", residual, M * cstore), ("out", out, M * cstore)):
        if t is None:
            continue
        if not t.is_contiguous():
            raise L.EdgeStyleHipError(f"conv_gemm: {what} must be contiguous (got shape {tuple(t.shape)}, strides {t.stride()})")
        if t.dtype != x.dtype or (numel is not None and t.numel() != numel):
            raise L.EdgeStyleHipError(f"conv_gemm: {what} has {t.numel()} {t.dtype} elements, the launch needs {numel} {x.dtype}")
    q = launch_query(M, Hout * Wout, pw, pws, group_n, src_numel=x.numel() * x_rep + (x2.numel() if x2 is not None else 0), stride=stride,
                     upsample=upsample, C1=C1, C2=C2, act=act, has_temb=temb is not None, has_residual=residual is not None,
                     unit_scale=out_scale == 1.0 and out_scale_dev is None, n_tails=len(tails), x_rep=x_rep, wide=wide, dtype=_dt(x),
                     gn_groups=gn_groups, force_splitk=splitk or 0, stages=stages)
    ch = L.LaunchChoice()
    if L.load().es_launch_choose(C.byref(q), C.byref(launch_knobs()), C.byref(ch)) != 0:
        raise L.EdgeStyleHipError(f"plan_gemm: rows_padded {pw.rows_padded} fits no N tile")
    if ch.route == L.ROUTE_LINEAR_XS:
        linear_xs(x.reshape(M, C1), pws if pws is not None else pw, M, out.reshape(M, cstore),
                  None if pws is None else [n * Hout * Wout for n in group_n],
                  residual=None if residual is None else residual.reshape(M, cstore))
        return out
    bn, splitk = ch.bn, ch.splitk
    d = L.GemmDesc()
    d.x, d.x2, d.w = x.data_ptr(), (x2.data_ptr() if x2 is not None else None), pw.w.data_ptr()
    d.bias = pw.bias.data_ptr() if pw.bias is not None else None
    d.temb = temb.data_ptr() if temb is not None else None
    d.residual = residual.data_ptr() if residual is not None else None
    d.out_scale_dev = out_scale_dev.data_ptr() if out_scale_dev is not None else None
    d.out = out.data_ptr()
    d.N, d.Hsrc, d.Wsrc, d.C1, d.C2 = N, H, W, C1, C2
    d.Hout, d.Wout, d.Cout = Hout, Wout, pw.cout
    d.rows_padded, d.Kpad = pw.rows_padded, pw.kpad
    d.ksize, d.stride, d.pad = k, stride, pad
    d.upsample = 1 if upsample else 0
    d.temb_stride = temb.stride(0) if temb is not None else 0
    d.act, d.splitk, d.bn, d.dtype, d.out_scale = act_i, splitk, bn, _dt(x), out_scale
    d.stages, d.waves, d.xcd_m_fastest = ch.stages, ch.waves, ch.xcd_m_fastest
    d.korder = pw.korder
    if ch.gn_partials:
        # the consumer of `out` is a GroupNorm over gn_groups groups: hand its statistics over from this launch's epilogue
        shape = (N, 2 * (Hout * Wout // 64), gn_groups, 2)
        part = gn_part if gn_part is not None else torch.empty(shape, dtype=torch.float32, device=x.device)
        if tuple(part.shape) != shape or part.dtype != torch.float32 or not part.is_contiguous():
            raise L.EdgeStyleHipError(f"conv_gemm: gn_part must be a contiguous fp32 {shape}")
        d.gn_part, d.gn_groups = part.data_ptr(), gn_groups
        out._gnp = (part, gn_groups)
    if ch.wide:
        # this launch adds into the residual stream: the sum over (residual hi + lo) in fp32, stored as hi + lo
        lo_in = getattr(residual, "_lo", None)
        if lo_in is not None:
            if lo_in.numel() != residual.numel() or not lo_in.is_contiguous():
                raise L.EdgeStyleHipError("conv_gemm: the residual's low part does not match it")
            d.residual_lo = lo_in.data_ptr()
        if out_lo is None:
            out_lo = torch.empty_like(out)
        elif out_lo.shape != out.shape or out_lo.dtype != out.dtype or not out_lo.is_contiguous():
            raise L.EdgeStyleHipError("conv_gemm: out_lo must match out")
        d.out_lo = out_lo.data_ptr()
        out._lo = out_lo
    d.x_nmod = nsrc if x_rep > 1 else 0
    if splitk > 1:
        ws = _get_workspace(splitk * M * pw.rows_padded * 4, x.device)
        d.workspace = ws.data_ptr()
    if pw.ln_colsum is not None:
        if (pws is not None and any(q.ln_colsum is None for q in pws)) or x2 is not None or k != 1:
            raise L.EdgeStyleHipError("LayerNorm-folded weights need a plain linear launch (all groups folded)")
        d.ln_colsum, d.ln_eps = pw.ln_colsum.data_ptr(), pw.ln_eps
    if tails:
        if any(t.shape[:3] != (N, Hout, Wout) or not t.is_contiguous() for t in tails):
            raise L.EdgeStyleHipError("conv_gemm: tail sources must be contiguous [N,Hout,Wout,C]")
        d.t1, d.Ct1 = tails[0].data_ptr(), tails[0].shape[3]
        if len(tails) == 2:
            d.t2, d.Ct2 = tails[1].data_ptr(), tails[1].shape[3]
    if pws is not None:
        hw = Hout * Wout
        gran = 256 if bn in (320, 256) else BM
        if len(pws) > 4 or len(group_n) != len(pws) or sum(group_n) != N or any((n * hw) % gran for n in group_n):
            raise L.EdgeStyleHipError(f"grouped conv_gemm: groups must cover N in whole {gran}-pixel tiles (<= 4 groups)")
        d.ngroups = len(pws)
        acc = 0
        for g, (q, n) in enumerate(zip(pws, group_n)):
            if (q.rows_padded, q.kpad, q.cout, q.cin, q.ksize, q.geglu, q.ctail, q.korder) != \
                    (pw.rows_padded, pw.kpad, pw.cout, pw.cin, pw.ksize, pw.geglu, pw.ctail, pw.korder):
                raise L.EdgeStyleHipError("grouped conv_gemm: weight geometry differs between groups")
            acc += n * hw // BM
            d.mt_end[g] = acc
            d.w_g[g] = q.w.data_ptr()
            d.bias_g[g] = q.bias.data_ptr() if q.bias is not None else None
            d.ln_colsum_g[g] = q.ln_colsum.data_ptr() if q.ln_colsum is not None else None
    if PROFILE is not None:           # bench.py roofline leg: in-kernel s_memrealtime stamps for this launch
        d.prof = PROFILE.next((2.0 * M * pw.cout * (k * k * (C1 + C2) + pw.ctail), k,
                               (M, pw.cout, k * k * (C1 + C2) + pw.ctail, stride, splitk, bn),
                               dict(N=N, H=H, W=W, C1=C1, C2=C2, cout=pw.cout, k=k, stride=stride, pad=pad,
                                    upsample=bool(upsample), geglu=pw.geglu, splitk=splitk, Hout=Hout, Wout=Wout,
                                    residual=residual is not None, temb=temb is not None, bn=bn,
                                    stages=int(d.stages), group_n=list(group_n) if pws is not None else None,
                                    ctail=pw.ctail,
                                    algorithmic_bytes=_algorithmic_bytes(x, x2, pw, pws, out, residual)
                                    + sum(t.numel() * t.element_size() for t in tails))))
        dd = L.GemmDesc()
        C.memmove(C.byref(dd), C.byref(d), C.sizeof(L.GemmDesc))
        dd.prof = None
        PROFILE.descs.append(dd)
    L.check(L.load().es_conv_gemm(C.byref(d), _stream()), "es_conv_gemm")
    return out


def _algorithmic_bytes(x, x2, pw, pws, out, residual) -> int:
    """HBM bytes a launch must move at least once: activations in, every weight set, output out, residual in."""
    n = x.numel() * x.element_size() + (x2.numel() * x2.element_size() if x2 is not None else 0)
    n += sum(q.w.numel() * q.w.element_size() for q in (pws if pws is not None else [pw]))
    n += out.numel() * out.element_size()
    if residual is not None:
        n += residual.numel() * residual.element_size()
    return int(n)


def linear(x: torch.Tensor, pw: PackedWeight, **kw) -> torch.Tensor:
    """x: [..., K] -> [..., Cout]; runs the same implicit-GEMM kernel with a 1x1 'image' of M pixels."""
    shp = x.shape
    M = x.numel() // shp[-1]
    out = kw.pop("out", None)
    res = kw.pop("residual", None)
    rep = kw.get("x_rep", 1)
    p0 = pw[0] if isinstance(pw, (list, tuple)) else pw
    cstore = p0.cout // 2 if p0.geglu else p0.cout
    y = conv_gemm(x.reshape(M, 1, 1, shp[-1]), pw,
                  residual=None if res is None else carry_lo(res.reshape(M * rep, 1, 1, cstore), res),
                  out=None if out is None else out.reshape(M * rep, 1, 1, cstore), **kw)
    if rep > 1:
        return carry_lo(y.reshape(shp[0] * rep, *shp[1:-1], cstore), y)
    return carry_lo(y.reshape(*shp[:-1], cstore), y)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q: [N,Sq,heads*d] view (any row stride), k/v: [N,Skv,heads*d] views -> [N,Sq,heads*d] contiguous.
    The launch takes data_ptr()s, one (N, heads, Sq, Skv, d) and the row and batch strides: whatever it would read or write differently
    from what the tensors hold is refused here, before anything is recorded or launched."""
    def bad(msg):
        return L.EdgeStyleHipError("attention: " + msg)
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise bad(f"q must be fp16 or bf16, not {q.dtype}")
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        raise bad("q, k, v must be [N, S, heads * d]")
    N, Sq, Cq = q.shape
    Skv = k.shape[1]
    if heads < 1 or Cq % heads != 0:
        raise bad(f"width {Cq} is not a multiple of heads {heads}")
    dh = Cq // heads
    if out is None:
        out = torch.empty((N, Sq, Cq), dtype=q.dtype, device=q.device)
    for name, t in (("k", k), ("v", v), ("out", out)):
        if t.dtype != q.dtype or t.device != q.device:
            raise bad(f"{name} is {t.dtype} on {t.device}, q is {q.dtype} on {q.device}")
    if k.shape != v.shape:
        raise bad(f"k {tuple(k.shape)} and v {tuple(v.shape)} differ")
    if k.shape[0] != N or k.shape[2] != Cq:
        raise bad(f"k / v {tuple(k.shape)} do not match q {tuple(q.shape)} in N or width")
    if out.dim() != 3 or out.shape != q.shape:
        raise bad(f"out {tuple(out.shape)} is not q's shape {tuple(q.shape)}")
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        if t.stride(2) != 1:
            raise bad("innermost stride must be 1")
        if t.stride(1) < Cq:
            raise bad(f"{name}: row stride {t.stride(1)} below the width {Cq}")
        unit = 8 if name == "out" else 16       # bytes: q, k, v are read as 16-byte vectors, out is written in 8-byte pieces
        es = t.element_size()
        if (t.stride(1) * es) % unit or (N > 1 and (t.stride(0) * es) % unit) or t.data_ptr() % unit:
            raise bad(f"{name}: row stride, batch stride and address must be multiples of {unit} bytes")
    d = L.AttnDesc()
    d.q, d.k, d.v, d.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    d.N, d.heads, d.Sq, d.Skv, d.d = N, heads, Sq, Skv, dh
    d.ldq, d.ldk, d.ldv, d.ldo = q.stride(1), k.stride(1), v.stride(1), out.stride(1)
    d.bsq, d.bsk, d.bsv, d.bso = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    d.scale = scale if scale is not None else 1.0 / math.sqrt(dh)
    d.dtype = _dt(q)
    L.check(L.load().es_attention(C.byref(d), _stream()), "es_attention")
    return out


_gn_partials = {}


def _norm_params(what, gamma, beta, Cc, x, nsets=None):
    """gamma / beta of a normalisation as lists of fp32 [Cc] tensors on x's device (the kernels read Cc floats behind each data_ptr())"""
    gl = list(gamma) if isinstance(gamma, (list, tuple)) else [gamma]
    bl = list(beta) if isinstance(beta, (list, tuple)) else [beta]
    if len(gl) != len(bl) or not gl or len(gl) > 4 or (nsets is not None and len(gl) != nsets):
        raise L.EdgeStyleHipError(f"{what}: {len(gl)} gamma and {len(bl)} beta sets" + (f" for {nsets} groups" if nsets is not None else " (1 to 4, as many of each)"))
    for name, ts in (("gamma", gl), ("beta", bl)):
        for t in ts:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != x.device or tuple(t.shape) != (Cc,) or not t.is_contiguous():
                raise L.EdgeStyleHipError(f"{what}: {name} must be a contiguous fp32 [{Cc}] tensor on {x.device}, not "
                                          f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
            if t.device.type != "meta" and t.data_ptr() % 16:         # gn_slab_kernel reads gamma / beta as 16-byte vectors
                raise L.EdgeStyleHipError(f"{what}: {name} must start at a multiple of 16 bytes (a slice at an odd offset of a larger buffer does not)")
    return gl, bl


def _gn_operands(what, x, x2, groups):
    """(N, H, W, C1, C2) of a GroupNorm launch whose sources the kernels can read as dense NHWC"""
    def bad(msg):
        return L.EdgeStyleHipError(f"{what}: {msg}")
    if x.dim() != 4 or x.dtype not in (torch.float16, torch.bfloat16):
        raise bad(f"x must be an fp16 or bf16 [N, H, W, C] tensor, not {x.dtype} {tuple(x.shape)}")
    N, H, W, C1 = x.shape
    if not x.is_contiguous():
        raise bad(f"x must be contiguous (got shape {tuple(x.shape)}, strides {x.stride()})")
    C2 = 0
    if x2 is not None:
        if x2.dtype != x.dtype or x2.device != x.device:
            raise bad(f"x2 is {x2.dtype} on {x2.device}, x is {x.dtype} on {x.device}")
        if x2.dim() != 4 or tuple(x2.shape[:3]) != (N, H, W):
            raise bad(f"x2 {tuple(x2.shape)} does not match x {tuple(x.shape)} in N, H, W")
        if not x2.is_contiguous():
            raise bad(f"x2 must be contiguous (got shape {tuple(x2.shape)}, strides {x2.stride()})")
        C2 = x2.shape[3]
    for name, t in (("x", x), ("x2", x2)):
        if t is not None and t.device.type != "meta" and t.data_ptr() % 16:
            raise bad(f"{name} must start at a multiple of 16 bytes (16-byte vector loads)")
    if N < 1 or H * W < 1 or C1 < 8 or C1 % 8 or C2 % 8:
        raise bad(f"channels {C1}+{C2} must be multiples of 8 (16-byte vector loads) and the problem not empty")
    if groups < 1 or (C1 + C2) % groups:
        raise bad(f"{C1 + C2} channels do not divide into {groups} groups")
    return N, H, W, C1, C2


def _gn_partials_for(what, x, N, groups, partials=None):
    if partials is None:
        key = (x.device, N, groups, LANE)
        partials = _gn_partials.get(key)
        if partials is None:
            partials = torch.empty(L.load().es_group_norm_partials_bytes(N, groups) // 4, dtype=torch.float32, device=x.device)
            _gn_partials[key] = partials
        return partials
    need = L.load().es_group_norm_partials_bytes(N, groups) // 4
    if partials.dtype != torch.float32 or partials.device != x.device or not partials.is_contiguous() or partials.numel() != need:
        raise L.EdgeStyleHipError(f"{what}: partials must be a contiguous fp32 tensor of {need} elements ([N][64][groups][2]) on {x.device}, not "
                                  f"{partials.dtype} {tuple(partials.shape)} on {partials.device}")
    return partials


def _norm_out(what, x, shape, out):
    if out is None:
        return torch.empty(shape, dtype=x.dtype, device=x.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise L.EdgeStyleHipError(f"{what}: out must be a contiguous {x.dtype} {tuple(shape)} tensor on {x.device}, not {out.dtype} {tuple(out.shape)} "
                                  f"(strides {out.stride()}) on {out.device}")
    if out.data_ptr() % 16:
        raise L.EdgeStyleHipError(f"{what}: out must start at a multiple of 16 bytes (16-byte vector stores)")
    return out


def group_norm(x: torch.Tensor, gamma, beta, groups: int, eps: float, silu: bool,
               x2: Optional[torch.Tensor] = None, group_n: Optional[Sequence[int]] = None,
               out: Optional[torch.Tensor] = None, partials: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x: [N,H,W,C1] (+x2 [N,H,W,C2]) -> normalised [N,H,W,C1+C2].  gamma/beta may be lists (one per group of
    `group_n` consecutive samples): one launch for several nets' GroupNorms.  out: the tensor to write (contiguous, x's dtype);
    partials: the statistics scratch (fp32, es_group_norm_partials_bytes(N, groups) bytes) instead of the cached one.  Operands the
    launch could not read as it is told to are refused here, before anything is recorded or launched."""
    N, H, W, C1, C2 = _gn_operands("group_norm", x, x2, groups)
    grouped = isinstance(gamma, (list, tuple)) and len(gamma) > 1
    if grouped and (len(gamma) > 4 or group_n is None or len(group_n) != len(gamma) or sum(group_n) != N):
        raise L.EdgeStyleHipError("grouped group_norm: bad group table")
    gl, bl = _norm_params("group_norm", gamma, beta, C1 + C2, x)
    out = _norm_out("group_norm", x, (N, H, W, C1 + C2), out)
    part = _gn_partials_for("group_norm", x, N, groups, partials)
    d = L.GnDesc()
    d.x, d.x2, d.out = x.data_ptr(), (x2.data_ptr() if x2 is not None else None), out.data_ptr()
    if grouped:
        d.ngroups = len(gl)
        acc = 0
        for g, n in enumerate(group_n):
            acc += n
            d.n_end[g] = acc
            d.gamma_g[g] = gl[g].data_ptr()
            d.beta_g[g] = bl[g].data_ptr()
        d.partials = part.data_ptr()
    else:
        d.gamma, d.beta, d.partials = gl[0].data_ptr(), bl[0].data_ptr(), part.data_ptr()
    gnp = getattr(x, "_gnp", None)
    if gnp is not None and partials is None and x2 is None and gn_handover(H * W, C1, groups) and gnp[1] == groups \
            and tuple(gnp[0].shape) == (N, 2 * (H * W // 64), groups, 2):
        d.partials, d.ext_chunks = gnp[0].data_ptr(), 2 * (H * W // 64)      # the producer's statistics: one streaming pass
    d.N, d.HW, d.C1, d.C2, d.groups = N, H * W, C1, C2, groups
    d.eps, d.silu, d.dtype = eps, 1 if silu else 0, _dt(x)
    L.check(L.load().es_group_norm(C.byref(d), _stream()), "es_group_norm")
    _drop_riders(out)
    return out


# Transformer2DModel.norm -> proj_in as ONE read of the tensor: a statistics pass (es_group_norm stats_only) and the projection on
# es_linear_xs, which normalises the rows it holds in registers (es_xs_desc.gn_part) - where the projection runs on that kernel anyway
# (the grouped launches of the two shallow levels, the UNet's own at batch 8), and at K = 320 from 8192 rows on, where the row-stationary
# kernel loses ~2 us to the tiled one but the apply pass it replaces costs 8-10 (profiles/r05_gn_proj_in.txt).  ES_GN_FOLD=0: two launches
# + projection as before.  The rule is the library's (es_launch_gn_fold): the native builder asks it too.
GN_FOLD = _os.environ.get("ES_GN_FOLD", "1") == "1"


def gn_fold_ok(M: int, hw: int, groups: int, pw: "PackedWeight", pws, group_n) -> bool:
    q = launch_query(M, hw, pw, pws, group_n)
    if pws is not None:             # (the fold wants ONE geometry too)
        q.groups_agree = all((p.rows_padded, p.kpad, p.cout, p.geglu, p.ln_colsum is None) == (pw.rows_padded, pw.kpad, pw.cout, pw.geglu, True) for p in pws)
    return bool(L.load().es_launch_gn_fold(C.byref(q), groups, C.byref(launch_knobs())))


def gn_proj_in(x: torch.Tensor, gamma, beta, groups: int, eps: float, pw, group_n: Optional[Sequence[int]] = None) -> torch.Tensor:
    """x [N,H,W,C] -> proj_in(GroupNorm(x)) [N,H,W,Cout] (no activation in between).  gamma / beta / pw: lists for a grouped launch
    (group_n samples each).  x, gamma and beta are held to what ops.group_norm demands, whichever form runs."""
    N, H, W, Cc, _ = _gn_operands("gn_proj_in", x, None, groups)
    pws = list(pw) if isinstance(pw, (list, tuple)) and len(pw) > 1 else None
    p0 = pw[0] if isinstance(pw, (list, tuple)) else pw
    gl, bl = _norm_params("gn_proj_in", gamma, beta, Cc, x, nsets=None if pws is None else len(pws))
    M, hw = N * H * W, H * W
    if not gn_fold_ok(M, hw, groups, p0, pws, group_n):
        kw = {} if group_n is None else dict(group_n=group_n)
        return conv_gemm(group_norm(x, gamma, beta, groups, eps, False, **kw), pw, **kw)
    part = _gn_partials_for("gn_proj_in", x, N, groups)
    d = L.GnDesc()
    d.x, d.partials = x.data_ptr(), part.data_ptr()
    d.N, d.HW, d.C1, d.C2, d.groups = N, hw, Cc, 0, groups
    d.eps, d.silu, d.dtype, d.stats_only = eps, 0, _dt(x), 1
    L.check(L.load().es_group_norm(C.byref(d), _stream()), "es_group_norm")
    out = torch.empty((N, H, W, p0.cout), dtype=x.dtype, device=x.device)
    linear_xs(x.reshape(M, Cc), pws if pws is not None else p0, M, out.reshape(M, p0.cout),
              None if pws is None else [n * hw for n in group_n],
              gn=dict(part=part, gamma=gl, beta=bl, groups=groups, nchunk=L.load().es_group_norm_chunks(hw), hw=hw, eps=eps))
    return out


def layer_norm(x: torch.Tensor, gamma, beta, eps: float = 1e-5, group_rows: Optional[Sequence[int]] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm over the last dimension of a contiguous x.  gamma / beta: fp32 [C], or lists with `group_rows` rows each.  out: the
    tensor to write (x's shape and dtype, contiguous).  Refused before anything is recorded or launched: what the launch cannot read."""
    if x.dim() < 1 or x.dtype not in (torch.float16, torch.bfloat16):
        raise L.EdgeStyleHipError(f"layer_norm: x must be an fp16 or bf16 [..., C] tensor, not {x.dtype} {tuple(x.shape)}")
    Cc = x.shape[-1]
    if not x.is_contiguous() or Cc < 8 or Cc % 8 or x.numel() < Cc:
        raise L.EdgeStyleHipError(f"layer_norm: x must be contiguous, not empty and C a multiple of 8 (got shape {tuple(x.shape)}, strides {x.stride()})")
    if x.device.type != "meta" and x.data_ptr() % 16:
        raise L.EdgeStyleHipError("layer_norm: x must start at a multiple of 16 bytes (16-byte vector loads)")
    M = x.numel() // Cc
    grouped = isinstance(gamma, (list, tuple)) and len(gamma) > 1
    if grouped and (len(gamma) > 4 or group_rows is None or len(group_rows) != len(gamma) or sum(group_rows) != M):
        raise L.EdgeStyleHipError("grouped layer_norm: bad group table")
    gl, bl = _norm_params("layer_norm", gamma, beta, Cc, x)
    if not L.load().es_layer_norm_route(Cc):
        raise L.EdgeStyleHipError(f"layer_norm: C = {Cc} > 4096 unsupported")
    out = _norm_out("layer_norm", x, tuple(x.shape), out)
    if grouped:
        d = L.LnDesc()
        d.x, d.out = x.data_ptr(), out.data_ptr()
        acc = 0
        for g, n in enumerate(group_rows):
            acc += n
            d.row_end[g] = acc
            d.gamma_g[g] = gl[g].data_ptr()
            d.beta_g[g] = bl[g].data_ptr()
        d.ngroups, d.M, d.C, d.eps, d.dtype = len(gl), M, Cc, eps, _dt(x)
        L.check(L.load().es_layer_norm_grouped(C.byref(d), _stream()), "es_layer_norm_grouped")
    else:
        L.check(L.load().es_layer_norm(_ptr(x), _ptr(out), _ptr(gl[0]), _ptr(bl[0]), M, Cc, eps, _dt(x), _stream()), "es_layer_norm")
    _drop_riders(out)
    return out


def timestep_embedding(t: torch.Tensor, dim: int, dtype) -> torch.Tensor:
    """t: fp32 device [N] -> [N, dim]"""
    N = t.numel()
    out = torch.empty((N, dim), dtype=dtype, device=t.device)
    L.check(L.load().es_timestep_embedding(_ptr(t), _ptr(out), N, dim, _DT[dtype], _stream()), "es_timestep_embedding")
    return out


def add(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if out is None:
        out = torch.empty_like(a)
    L.check(L.load().es_add(_ptr(a), _ptr(b), _ptr(out), a.numel(), _dt(a), _stream()), "es_add")
    _drop_riders(out)
    return out


def _drop_riders(t: torch.Tensor):
    """A tensor written in place no longer matches what rides on its Python object: the low word of the two-word residual stream
    (`._lo`) and the GroupNorm statistics its producer handed over (`._gnp`) describe the OLD contents."""
    for name in ("_lo", "_gnp"):
        if hasattr(t, name):
            delattr(t, name)


def nchw_to_nhwc(x: torch.Tensor, dtype, cpad: Optional[int] = None) -> torch.Tensor:
    """fp32 NCHW (contiguous, device) -> NHWC dtype with channels zero-padded to cpad."""
    N, Cc, H, W = x.shape
    cp = cpad or Cc
    x = x.contiguous().float()
    out = torch.empty((N, H, W, cp), dtype=dtype, device=x.device)
    L.check(L.load().es_nchw_f32_to_nhwc(_ptr(x), _ptr(out), N, Cc, H * W, cp, _DT[dtype], _stream()),
            "es_nchw_f32_to_nhwc")
    return out


def nhwc_to_nchw(x: torch.Tensor, channels: Optional[int] = None, scale: float = 1.0, shift: float = 0.0,
                 clamp01: bool = False) -> torch.Tensor:
    """NHWC dtype -> fp32 NCHW, optionally y = clamp(x*scale+shift, 0, 1) (image postprocess PL:570-572)."""
    N, H, W, Cs = x.shape
    Cc = channels or Cs
    out = torch.empty((N, Cc, H, W), dtype=torch.float32, device=x.device)
    L.check(L.load().es_nhwc_to_nchw_f32(_ptr(x), _ptr(out), N, Cc, H * W, Cs, scale, shift, 1 if clamp01 else 0,
                                         _dt(x), _stream()), "es_nhwc_to_nchw_f32")
    return out


def vae_sample(moments: torch.Tensor, noise_nchw: torch.Tensor, latent: int, lpad: int, scaling: float):
    N, H, W, _ = moments.shape
    z = torch.empty((N, H, W, lpad), dtype=moments.dtype, device=moments.device)
    L.check(L.load().es_vae_sample(_ptr(moments), _ptr(noise_nchw.contiguous().float()), _ptr(z), N, H * W, latent,
                                   lpad, scaling, _dt(moments), _stream()), "es_vae_sample")
    return z


def cfg_ddim_step(noise: torch.Tensor, latents: torch.Tensor, model_in: torch.Tensor, coef: torch.Tensor,
                  step_idx: torch.Tensor, guidance_scale: float, cfg: bool):
    """noise [2B|B,H,W,L] dtype; latents fp32 [B,H,W,L] (in place); model_in [2B|B,H,W,Ls] dtype (rewritten)."""
    B, H, W, Lc = latents.shape
    L.check(L.load().es_cfg_ddim_step(_ptr(noise), _ptr(latents), _ptr(model_in), _ptr(coef), _ptr(step_idx),
                                      guidance_scale, B, H * W, Lc, model_in.shape[3], 1 if cfg else 0, coef.shape[0],
                                      _dt(noise), _stream()), "es_cfg_ddim_step")


def cfg_unipc_step(noise, latents, last_sample, m0, m1, model_in, coef, step_idx, guidance_scale: float, cfg: bool):
    """UniPC counterpart of cfg_ddim_step; last_sample/m0/m1 are fp32 [B,H,W,L] state tensors (in place)."""
    B, H, W, Lc = latents.shape
    L.check(L.load().es_cfg_unipc_step(_ptr(noise), _ptr(latents), _ptr(last_sample), _ptr(m0), _ptr(m1),
                                       _ptr(model_in), _ptr(coef), _ptr(step_idx), guidance_scale, B, H * W, Lc,
                                       model_in.shape[3], 1 if cfg else 0, coef.shape[0], _dt(noise), _stream()),
            "es_cfg_unipc_step")


def memcpy(dst: torch.Tensor, src: torch.Tensor):
    """dst[:] = src, both contiguous device tensors of equal byte size (a C-ABI call: part of recorded plans)."""
    nb = src.numel() * src.element_size()
    if not (dst.is_contiguous() and src.is_contiguous()) or dst.numel() * dst.element_size() != nb:
        raise L.EdgeStyleHipError("memcpy: contiguous tensors of equal byte size")
    L.check(L.load().es_memcpy(_ptr(dst), _ptr(src), nb, _stream()), "es_memcpy")
    _drop_riders(dst)


def memcpy2d(dst_ptr: int, dpitch: int, src_ptr: int, spitch: int, width: int, height: int):
    """`height` rows of `width` bytes, pitches in bytes (src pitch 0 = broadcast one row is NOT supported: use height 1)."""
    L.check(L.load().es_memcpy2d(C.c_void_p(dst_ptr), dpitch, C.c_void_p(src_ptr), spitch, width, height, _stream()),
            "es_memcpy2d")


def fill_f32(dst: torch.Tensor, value: float):
    L.check(L.load().es_fill_f32(_ptr(dst), float(value), dst.numel(), _stream()), "es_fill_f32")


def latents_to_input(latents: torch.Tensor, model_in: torch.Tensor, cfg: bool):
    """latents fp32 [B,H,W,L] -> model_in [2B|B,H,W,Ls] compute dtype, channel-padded, both CFG halves (PL:443-447)."""
    B, H, W, Lc = latents.shape
    L.check(L.load().es_latents_to_input(_ptr(latents), _ptr(model_in), B, H * W, Lc, model_in.shape[3], 1 if cfg else 0,
                                         _dt(model_in), _stream()), "es_latents_to_input")


def incr(ctr: torch.Tensor):
    L.check(L.load().es_incr(_ptr(ctr), _stream()), "es_incr")


def gather_row(table: torch.Tensor, idx: torch.Tensor, out: torch.Tensor):
    """out[:] = table[idx[0]] (fp32), selected on the device"""
    L.check(L.load().es_gather_row(_ptr(table), _ptr(idx), _ptr(out), out.numel(), table.shape[0], _stream()),
            "es_gather_row")


_fusion_scratch = {}
_FUSION_PLANES = (("g1", 3), ("be1", 3), ("g2", 1), ("be2", 1))
_FUSION_VECTORS = (("w1", 6), ("b1", 3), ("w2", 3), ("b2", 1), ("w3", 1), ("b3", 1))


def _fusion_check(res, res_bs, params: dict, N: int, HW: int, Cc: int, scales_dev, out, addend=None):
    """The library gets data_ptr()s, N, HW, C and six batch strides: everything it will read or write is checked here, before a
    descriptor exists.  A residual may be a view into a batched buffer ([n >= N, ...] with any batch stride >= HW * C); inside a
    sample it is dense."""
    def refuse(msg):
        raise L.EdgeStyleHipError("fusion_block: " + msg)
    if len(res) != 6 or len(res_bs) != 6:
        refuse("six residuals and six batch strides")
    if N < 1 or HW < 1 or Cc < 8 or Cc % 8:
        refuse(f"N {N}, HW {HW}, C {Cc}: C must be a positive multiple of 8")
    dt, per = res[0].dtype, HW * Cc
    if dt not in _DT:
        refuse(f"residual dtype {dt} (fp16 or bf16)")
    for i, (t, bs) in enumerate(zip(res, res_bs)):
        name = f"residual {i} "
        if t.dtype != dt:
            refuse(name + f"has dtype {t.dtype}, residual 0 has {dt}")
        if t.dim() < 2 or t.shape[0] < 1 or t[0].numel() != per or not t[0].is_contiguous():
            refuse(name + f"of shape {tuple(t.shape)}, strides {tuple(t.stride())} is not dense [n, HW * C = {per}] inside a sample")
        bs = int(bs)
        if bs < per:
            refuse(name + f"batch stride {bs} < HW * C = {per}")
        if bs % 8 or t.data_ptr() % 16:
            refuse(name + f"is read in 16-byte pieces: batch stride {bs} must be a multiple of 8 elements, the address of 16 bytes")
        if t.shape[0] > 1 and bs != t.stride(0):
            refuse(name + f"batch stride {bs} is not the view's ({t.stride(0)})")
        if (t.shape[0] - 1) * (t.stride(0) if t.shape[0] > 1 else 0) + per < (N - 1) * bs + per:
            refuse(name + f"holds {t.shape[0]} samples at stride {t.stride(0)}: fewer than (N - 1) * {bs} + {per} elements")
    for name, k in _FUSION_PLANES:
        t = params[name]
        if t.dtype != dt or t.numel() != per * k or not t.is_contiguous():
            refuse(f"{name} must be a contiguous {dt} plane of HW * C * {k} = {per * k} values (got {t.dtype}, {t.numel()})")
    for name, k in _FUSION_VECTORS:
        t = params[name]
        if t.dtype != torch.float32 or t.numel() != Cc * k or not t.is_contiguous():
            refuse(f"{name} must hold C * {k} = {Cc * k} contiguous fp32 values (got {t.dtype}, {t.numel()})")
    for name, t in (("out", out), ("addend", addend)):
        if t is not None and (t.numel() != N * per or not t.is_contiguous() or t.dtype != dt
                              or (name == "out" and tuple(t.shape) != (N, HW, Cc))):
            refuse(f"{name} must be a contiguous [N, HW, C] tensor of the compute dtype (got {tuple(t.shape)}, {t.dtype})")
    if scales_dev is not None and (scales_dev.dtype != torch.float32 or scales_dev.numel() < 6 or not scales_dev.is_contiguous()):
        refuse("scales_dev must hold 6 contiguous fp32 values")


def _fusion_desc(res, res_bs, params: dict, N: int, HW: int, Cc: int, scales, scales_dev, out, eps, slot: int,
                 addend: Optional[torch.Tensor] = None):
    t0 = res[0]
    _fusion_check(res, res_bs, params, N, HW, Cc, scales_dev, out, addend)
    key = (t0.device, N, slot)
    sc = _fusion_scratch.get(key)
    if sc is None:
        sc = torch.empty(L.load().es_fusion_scratch_bytes(N) // 4, dtype=torch.float32, device=t0.device)
        _fusion_scratch[key] = sc
    u = torch.empty((N, HW, Cc), dtype=t0.dtype, device=t0.device)
    if out is None:
        out = torch.empty((N, HW, Cc), dtype=t0.dtype, device=t0.device)
    d = L.FusionDesc()
    for i in range(6):
        d.res[i] = res[i].data_ptr()
        d.res_bs[i] = res_bs[i]
        d.res_scale[i] = float(scales[i])
    d.res_scale_dev = scales_dev.data_ptr() if scales_dev is not None else None
    for name in ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "w3", "b3"):
        setattr(d, name, params[name].data_ptr())
    d.scratch, d.u, d.out = sc.data_ptr(), u.data_ptr(), out.data_ptr()
    d.N, d.HW, d.C, d.eps, d.dtype = N, HW, Cc, eps, _dt(t0)
    if addend is not None:
        d.addend = addend.data_ptr()
    return d, u, out


def fusion_block(res, res_bs, params: dict, N: int, HW: int, Cc: int, scales, scales_dev=None,
                 out: Optional[torch.Tensor] = None, eps: float = 1e-5) -> torch.Tensor:
    """res: 6 tensors (or views) whose data_ptr() is sample 0 of net i; res_bs: 6 batch strides (elements)."""
    d, _u, out = _fusion_desc(res, res_bs, params, N, HW, Cc, scales, scales_dev, out, eps, 0)
    L.check(L.load().es_fusion_block(C.byref(d), _stream()), "es_fusion_block")
    return out


def fusion_blocks(blocks, N: int, scales, scales_dev=None, eps: float = 1e-5, addends=None, first_block: int = 0):
    """All fusion blocks of a step in three launches.  blocks: list of (res, res_bs, params, HW, Cc) as for
    fusion_block; returns the list of [N,HW,Cc] outputs.  addends: optional list of [N,HW,Cc] tensors added to the
    outputs (the UNet skip tensors: saves the 13 separate adds of PL:500-510)."""
    keep, outs = [], []
    for k, (res, res_bs, params, HW, Cc) in enumerate(blocks):       # all of them before the first launch
        _fusion_check(res, res_bs, params, N, HW, Cc, scales_dev, None, None if addends is None else addends[k])
    for k0 in range(0, len(blocks), L.FUSION_MAX_BATCH):
        part = blocks[k0:k0 + L.FUSION_MAX_BATCH]
        arr = (L.FusionDesc * len(part))()
        for k, (res, res_bs, params, HW, Cc) in enumerate(part):
            d, u, out = _fusion_desc(res, res_bs, params, N, HW, Cc, scales, scales_dev, None, eps, first_block + k0 + k,
                                     None if addends is None else addends[k0 + k])
            arr[k] = d
            keep.append(u)
            outs.append(out)
        L.check(L.load().es_fusion_blocks(arr, len(part), _stream()), "es_fusion_blocks")
    return outs


def pack_fusion_params(sd: dict, prefix: str, dtype, device) -> dict:
    """Repack one ControlNetBlock (MC:23-53) pixel-major for es_fusion_block."""
    w1 = sd[f"{prefix}.first_conv.weight"].float()            # [3C, 2, 1, 1], out channel j = 3c + p
    c3 = w1.shape[0]
    c = c3 // 3
    g1 = sd[f"{prefix}.first_normalization.weight"].float()   # [3C, H, W]
    hw = g1.shape[1] * g1.shape[2]

    def plane3(t):   # [3C,H,W] -> [HW, C, 3]
        return t.reshape(c, 3, hw).permute(2, 0, 1).contiguous()

    def plane1(t):   # [C,H,W] -> [HW, C]
        return t.reshape(c, hw).permute(1, 0).contiguous()

    p = {
        "w1": w1.reshape(c, 3, 2).contiguous(),
        "b1": sd[f"{prefix}.first_conv.bias"].float().reshape(c, 3).contiguous(),
        "g1": plane3(g1).to(dtype), "be1": plane3(sd[f"{prefix}.first_normalization.bias"].float()).to(dtype),
        "w2": sd[f"{prefix}.second_conv.weight"].float().reshape(c, 3).contiguous(),
        "b2": sd[f"{prefix}.second_conv.bias"].float().contiguous(),
        "g2": plane1(sd[f"{prefix}.second_normalization.weight"].float()).to(dtype),
        "be2": plane1(sd[f"{prefix}.second_normalization.bias"].float()).to(dtype),
        "w3": sd[f"{prefix}.third_conv.weight"].float().reshape(c).contiguous(),
        "b3": sd[f"{prefix}.third_conv.bias"].float().contiguous(),
    }
    return {k: v.to(device) for k, v in p.items()}


# ----------------------------------------------------------------------------------------------------------------
# byte images (csrc/image_io.hip): Pillow-exact resize + centre crop, bytes -> network input, network output -> bytes
# ----------------------------------------------------------------------------------------------------------------
def image_descriptors(images: Sequence[torch.Tensor], what: str = "image_resize_u8"):
    """uint8 HWC device tensors ([H,W,3|4]; rows may be pitched: stride(0) >= W * channels bytes) -> an es_image_u8 array.
    The library gets data_ptr(), height, width, channels and the row stride: whatever it would read differently from what the
    tensors hold is refused here."""
    def bad(msg):
        return L.EdgeStyleHipError(f"{what}: {msg}")
    if len(images) < 1:
        raise bad("no images")
    arr = (L.ImageU8 * len(images))()
    dev = images[0].device
    for i, t in enumerate(images):
        if not torch.is_tensor(t) or t.dtype != torch.uint8:
            raise bad(f"image {i} must be a uint8 tensor")
        if not t.is_cuda or t.device != dev:
            raise bad(f"image {i} is on {t.device}: all images must be on one GPU")
        if t.dim() != 3 or t.shape[2] not in (3, 4) or t.shape[0] < 1 or t.shape[1] < 1:
            raise bad(f"image {i} must be [H, W, 3 | 4] (HWC), got {tuple(t.shape)}")
        H, W, ch = t.shape
        if t.stride(2) != 1 or t.stride(1) != ch or (H > 1 and t.stride(0) < W * ch):
            raise bad(f"image {i}: pixels must be dense and the row stride at least width * channels (strides {t.stride()})")
        arr[i].data, arr[i].height, arr[i].width, arr[i].channels = t.data_ptr(), H, W, ch
        arr[i].row_stride = t.stride(0) if H > 1 else W * ch
    return arr


def image_resize_workspace_bytes(descs, R: int) -> int:
    return int(L.load().es_image_resize_workspace_bytes(descs, len(descs), int(R)))


def image_resize_u8(images: Sequence[torch.Tensor], R: int, out: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torchvision Resize(R, BILINEAR) on a PIL image -> CenterCrop(R) for a list of uint8 HWC device tensors of any sizes,
    as ONE call: -> uint8 [count, R, R, 3], byte for byte Pillow's pixels (TT:29-48)."""
    def bad(msg):
        return L.EdgeStyleHipError("image_resize_u8: " + msg)
    if int(R) < 1:
        raise bad("R < 1")
    R = int(R)
    descs = image_descriptors(images)
    n, dev = len(images), images[0].device
    if out is None:
        out = torch.empty((n, R, R, 3), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.device != dev or tuple(out.shape) != (n, R, R, 3) or not out.is_contiguous():
        raise bad(f"out must be a contiguous uint8 [{n}, {R}, {R}, 3] tensor on {dev}")
    need = image_resize_workspace_bytes(descs, R)
    if workspace is None:
        workspace = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need:
        raise bad(f"workspace must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
    L.check(L.load().es_image_resize_u8(descs, n, _ptr(out), R, _ptr(workspace), workspace.numel(), _stream()), "es_image_resize_u8")
    return out


def image_u8_to_f32(x: torch.Tensor, normalize: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ToTensor (+ Normalize(.5, .5)): uint8 HWC [count,H,W,3] -> fp32 NCHW [count,3,H,W] in [0,1] ([-1,1] if normalize)."""
    def bad(msg):
        return L.EdgeStyleHipError("image_u8_to_f32: " + msg)
    if x.dtype != torch.uint8 or not x.is_cuda:
        raise bad(f"x must be a uint8 device tensor, not {x.dtype} on {x.device}")
    if x.dim() != 4 or x.shape[3] != 3 or min(x.shape) < 1:
        raise bad(f"x must be [count, H, W, 3], got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise bad("x must be dense")
    n, H, W, _ = x.shape
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or out.device != x.device or tuple(out.shape) != (n, 3, H, W) or not out.is_contiguous():
        raise bad(f"out must be a contiguous fp32 [{n}, 3, {H}, {W}] tensor on {x.device}")
    L.check(L.load().es_image_u8_to_f32(_ptr(x), _ptr(out), n, H, W, 1 if normalize else 0, _stream()), "es_image_u8_to_f32")
    return out


def image_f32_to_u8(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 NCHW [B,3,H,W] in [0,1] -> uint8 HWC [B,H,W,3] = (x * 255).round() clamped to 0..255 (PL:570-572's "pil" rounding)."""
    def bad(msg):
        return L.EdgeStyleHipError("image_f32_to_u8: " + msg)
    if x.dtype != torch.float32 or not x.is_cuda:
        raise bad(f"x must be an fp32 device tensor, not {x.dtype} on {x.device}")
    if x.dim() != 4 or x.shape[1] != 3 or min(x.shape) < 1:
        raise bad(f"x must be [B, 3, H, W], got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise bad("x must be dense")
    B, _, H, W = x.shape
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=x.device)
    elif out.dtype != torch.uint8 or out.device != x.device or tuple(out.shape) != (B, H, W, 3) or not out.is_contiguous():
        raise bad(f"out must be a contiguous uint8 [{B}, {H}, {W}, 3] tensor on {x.device}")
    L.check(L.load().es_image_f32_to_u8(_ptr(x), _ptr(out), B, H, W, _stream()), "es_image_f32_to_u8")
    return out


def person_crop_fit(height: int, width: int, box, final_width: int = 512, final_height: int = 512, margin: float = 0.1):
    """create_processed_image's geometry (extract_dataset.py:118-164) -> (new_w, new_h, left, top); left / top may be negative"""
    out = (C.c_int32 * 4)()
    b = (C.c_double * 4)(*[float(v) for v in box])
    L.check(L.load().es_person_crop_fit(int(height), int(width), b, int(final_width), int(final_height), float(margin), out), "es_person_crop_fit")
    return tuple(out)


def _u8_out_and_workspace(what, out, shape, need, workspace, dev):
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.device != dev or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise L.EdgeStyleHipError(f"{what}: out must be a contiguous uint8 {list(shape)} tensor on {dev}")
    if workspace is None:
        workspace = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need:
        raise L.EdgeStyleHipError(f"{what}: workspace must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
    return out, workspace


def image_resize_window_u8(images: Sequence[torch.Tensor], geom, out_h: int, out_w: int, filter: int = L.FILTER_LANCZOS,
                           out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Each uint8 HWC device image resized to geom[i] = (new_w, new_h, left, top)'s size with Pillow's `filter`, of which the out_h x out_w
    window at (top, left) is kept (zeros where it hangs outside), as ONE call: -> uint8 [count, out_h, out_w, 3]."""
    what = "image_resize_window_u8"
    descs = image_descriptors(images, what)
    n, dev = len(images), images[0].device
    flat = [int(v) for g in geom for v in g]
    if len(flat) != 4 * n:
        raise L.EdgeStyleHipError(f"{what}: geom must hold (new_w, new_h, left, top) for each of the {n} images")
    g = (C.c_int32 * (4 * n))(*flat)
    lib = L.load()
    need = int(lib.es_image_resize_window_u8_workspace_bytes(descs, n, g, int(out_h), int(out_w), int(filter)))
    out, workspace = _u8_out_and_workspace(what, out, (n, int(out_h), int(out_w), 3), need, workspace, dev)
    L.check(lib.es_image_resize_window_u8(descs, n, g, _ptr(out), int(out_h), int(out_w), int(filter), _ptr(workspace), workspace.numel(), _stream()),
            "es_image_resize_window_u8")
    return out


def person_crop_u8(images: Sequence[torch.Tensor], boxes, out: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """create_processed_image (extract_dataset.py:112-171) for a list of uint8 HWC device photos and their person boxes
    (xmin, ymin, xmax, ymax) as ONE call: -> uint8 [count, 512, 512, 3]."""
    what = "person_crop_u8"
    descs = image_descriptors(images, what)
    n, dev = len(images), images[0].device
    flat = [float(v) for b in boxes for v in b]
    if len(flat) != 4 * n:
        raise L.EdgeStyleHipError(f"{what}: boxes must hold (xmin, ymin, xmax, ymax) for each of the {n} images")
    b = (C.c_double * (4 * n))(*flat)
    lib = L.load()
    out4 = (C.c_int32 * 4)()
    for i in range(n):                                     # (a refused box is reported before anything is allocated)
        L.check(lib.es_person_crop_fit(descs[i].height, descs[i].width, (C.c_double * 4)(*flat[4 * i:4 * i + 4]), 512, 512, 0.1, out4),
                "es_person_crop_fit")
    need = int(lib.es_person_crop_u8_workspace_bytes(descs, n, b))
    out, workspace = _u8_out_and_workspace(what, out, (n, 512, 512, 3), need, workspace, dev)
    L.check(lib.es_person_crop_u8(descs, n, b, _ptr(out), _ptr(workspace), workspace.numel(), _stream()), "es_person_crop_u8")
    return out


def pose_draw(keypoints: torch.Tensor, H: int, W: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """draw_poses(.., draw_body=True) on black canvases (csrc/pose.hip): fp32 device key points [count, 18, 3] = (x, y, score), x and y in
    [0, 1], score not > 0 = absent -> uint8 [count, H, W, 3], one launch."""
    what = "pose_draw"
    kp = keypoints
    if not torch.is_tensor(kp) or kp.dtype != torch.float32 or not kp.is_cuda:
        raise L.EdgeStyleHipError(f"{what}: keypoints must be an fp32 device tensor")
    if kp.dim() != 3 or tuple(kp.shape[1:]) != (18, 3) or kp.shape[0] < 1 or not kp.is_contiguous():
        raise L.EdgeStyleHipError(f"{what}: keypoints must be a dense [count, 18, 3] tensor, got {tuple(kp.shape)}")
    n, H, W = kp.shape[0], int(H), int(W)
    if H < 1 or W < 1:
        raise L.EdgeStyleHipError(f"{what}: H or W < 1")
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=kp.device)
    elif out.dtype != torch.uint8 or out.device != kp.device or tuple(out.shape) != (n, H, W, 3) or not out.is_contiguous():
        raise L.EdgeStyleHipError(f"{what}: out must be a contiguous uint8 [{n}, {H}, {W}, 3] tensor on {kp.device}")
    L.check(L.load().es_pose_draw(_ptr(kp), _ptr(out), n, H, W, _stream()), "es_pose_draw")
    return out


# ----------------------------------------------------------------------------------------------------------------
# JPEG reconstruction (csrc/jpeg.hip): quantised DCT coefficients -> RGB bytes.  The host half (headers, Huffman decoding) is wrapped in
# edgestyle_amd/jpeg.py, which also owns the convenient entry points; these two take what it prepared.
# ----------------------------------------------------------------------------------------------------------------
def _jpeg_outputs(what, infos, out, dev):
    n = len(infos)
    if out is None:
        out = [torch.empty((infos[i].height, infos[i].width, 3), dtype=torch.uint8, device=dev) for i in range(n)]
    if len(out) != n:
        raise L.EdgeStyleHipError(f"{what}: {n} outputs expected")
    descs = (L.ImageU8 * n)()
    for i, t in enumerate(out):
        H, W = infos[i].height, infos[i].width
        if (not torch.is_tensor(t) or t.dtype != torch.uint8 or t.device != dev or tuple(t.shape) != (H, W, 3) or t.stride(2) != 1
                or t.stride(1) != 3 or (H > 1 and t.stride(0) < W * 3)):
            raise L.EdgeStyleHipError(f"{what}: output {i} must be a uint8 [{H}, {W}, 3] tensor on {dev} with dense pixels")
        descs[i].data, descs[i].height, descs[i].width, descs[i].channels = t.data_ptr(), H, W, 3
        descs[i].row_stride = t.stride(0) if H > 1 else W * 3
    return out, descs


def _jpeg_bytes_buffer(what, t, need, dev, name):
    if t is None:
        return torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    if t.dtype != torch.uint8 or t.device != dev or not t.is_contiguous() or t.numel() < need:
        raise L.EdgeStyleHipError(f"{what}: {name} must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
    return t


def jpeg_reconstruct(infos, coeffs: Sequence[torch.Tensor], qtables: Sequence[torch.Tensor], out=None,
                     workspace: Optional[torch.Tensor] = None):
    """infos: an array of L.JpegInfo; coeffs[i] / qtables[i]: device int16 tensors holding what es_jpeg_entropy_decode_host wrote for image
    i (the tables' uint16 values as their int16 bit patterns).  -> a list of uint8 [H, W, 3] device tensors (`out`, when given: rows may
    be pitched).  Images of different sizes and samplings are ONE call: two launches per 16 images."""
    what = "jpeg_reconstruct"
    n = len(infos)
    if n < 1 or len(coeffs) != n or len(qtables) != n:
        raise L.EdgeStyleHipError(f"{what}: one coefficient and one table tensor per image expected")
    dev = coeffs[0].device
    lib = L.load()
    for i in range(n):
        for t, count, name in ((coeffs[i], int(lib.es_jpeg_coeff_count(C.byref(infos[i]))), "coefficients"), (qtables[i], 64 * infos[i].components, "tables")):
            if count == 0:
                L.check(-1, "es_jpeg_coeff_count")
            if not torch.is_tensor(t) or t.dtype != torch.int16 or t.device != dev or not t.is_cuda or not t.is_contiguous() or t.numel() < count:
                raise L.EdgeStyleHipError(f"{what}: {name} {i} must be a contiguous int16 device tensor of at least {count} values")
    need = int(lib.es_jpeg_reconstruct_workspace_bytes(infos, n))
    if need == 0:
        L.check(-1, "es_jpeg_reconstruct_workspace_bytes")
    out, descs = _jpeg_outputs(what, infos, out, dev)
    workspace = _jpeg_bytes_buffer(what, workspace, need, dev, "workspace")
    cp = (C.c_void_p * n)(*[t.data_ptr() for t in coeffs])
    qp = (C.c_void_p * n)(*[t.data_ptr() for t in qtables])
    L.check(lib.es_jpeg_reconstruct(infos, n, cp, qp, descs, _ptr(workspace), workspace.numel(), _stream()), "es_jpeg_reconstruct")
    return out


def jpeg_decode_u8(datas: Sequence[bytes], infos, device, out=None, staging_host: Optional[torch.Tensor] = None,
                   staging_dev: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """es_jpeg_decode_u8: parse + upload + reconstruct of up to 64 files (bytes objects; infos: their L.JpegInfo array) in one call ->
    a list of uint8 [H, W, 3] tensors on `device`.  staging_host: a pinned uint8 host tensor the caller keeps untouched until the stream has
    passed the upload; when None one is allocated and the call waits for the stream before it returns."""
    what = "jpeg_decode_u8"
    n = len(datas)
    if n < 1 or len(infos) != n:
        raise L.EdgeStyleHipError(f"{what}: one info per file expected")
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    lib = L.load()
    stage, need = int(lib.es_jpeg_decode_staging_bytes(infos, n)), int(lib.es_jpeg_reconstruct_workspace_bytes(infos, n))
    if stage == 0 or need == 0:
        L.check(-1, "es_jpeg_decode_staging_bytes")
    out, descs = _jpeg_outputs(what, infos, out, dev)
    own = staging_host is None
    if own:
        staging_host = torch.empty((stage,), dtype=torch.uint8, pin_memory=True)
    elif staging_host.dtype != torch.uint8 or staging_host.is_cuda or not staging_host.is_contiguous() or staging_host.numel() < stage:
        raise L.EdgeStyleHipError(f"{what}: staging_host must be a contiguous uint8 host tensor of at least {stage} bytes")
    staging_dev = _jpeg_bytes_buffer(what, staging_dev, stage, dev, "staging_dev")
    workspace = _jpeg_bytes_buffer(what, workspace, need, dev, "workspace")
    bp = (C.c_void_p * n)(*[C.cast(C.c_char_p(d), C.c_void_p) for d in datas])
    ln = (C.c_size_t * n)(*[len(d) for d in datas])
    L.check(lib.es_jpeg_decode_u8(bp, ln, n, descs, C.c_void_p(staging_host.data_ptr()), _ptr(staging_dev), min(staging_host.numel(), staging_dev.numel()),
                                  _ptr(workspace), workspace.numel(), _stream()), "es_jpeg_decode_u8")
    if own:                                       # the upload reads the staging memory on the stream: it must not be freed before
        torch.cuda.current_stream().synchronize()
    return out


# ----------------------------------------------------------------------------------------------------------------
# Huffman decoding on the device (csrc/jpeg_entropy.hip), opt-in: the default decoder is still the host one above.  The host half
# (es_jpeg_scan_prepare_host) is wrapped in edgestyle_amd/jpeg.py; these take what it prepared.
# ----------------------------------------------------------------------------------------------------------------
def jpeg_status_check(status: torch.Tensor, what="jpeg"):
    """reads the status words back (this waits for the stream) and raises EdgeStyleHipError with the text of the first defect"""
    words = status.cpu().tolist()
    for i, code in enumerate(words):
        if code != 0:
            text = L.load().es_jpeg_status_text(int(code)).decode()
            raise L.EdgeStyleHipError(f"{what}: image {i}: {text} (status {code})")


def jpeg_entropy_decode(infos, files: Sequence[torch.Tensor], segments: Sequence[torch.Tensor], tables: Sequence[torch.Tensor], subseq_bytes: int = 0,
                        coeffs=None, status: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """es_jpeg_entropy_decode.  infos: an array of L.JpegInfo; files[i]: device uint8 tensor holding file i (all of it is readable; the
    segments' offsets are cut to its length); segments[i]: device int32 tensor, the pairs es_jpeg_scan_prepare_host wrote; tables[i]:
    device uint8 tensor of L.JPEG_TABLES_BYTES.  -> (a list of int16 coefficient tensors, the int32 status tensor [n]), nothing is read
    back.  Images of different sizes, samplings and segment counts are ONE call: two launches per 16 images."""
    what = "jpeg_entropy_decode"
    n = len(infos)
    if n < 1 or len(files) != n or len(segments) != n or len(tables) != n:
        raise L.EdgeStyleHipError(f"{what}: one file, one segment and one table tensor per image expected")
    dev = files[0].device
    lib = L.load()
    counts = [int(lib.es_jpeg_coeff_count(C.byref(infos[i]))) for i in range(n)]
    nseg = [int(lib.es_jpeg_segment_count(C.byref(infos[i]))) for i in range(n)]
    if 0 in counts or 0 in nseg:
        L.check(-1, "es_jpeg_coeff_count")
    for i in range(n):
        for t, dtype, least, name in ((files[i], torch.uint8, 1, "file"), (segments[i], torch.int32, 2 * nseg[i], "segments"),
                                      (tables[i], torch.uint8, L.JPEG_TABLES_BYTES, "tables")):
            if not torch.is_tensor(t) or t.dtype != dtype or t.device != dev or not t.is_cuda or not t.is_contiguous() or t.numel() < least:
                raise L.EdgeStyleHipError(f"{what}: {name} {i} must be a contiguous {dtype} device tensor of at least {least} values")
    if coeffs is None:
        coeffs = [torch.empty((c,), dtype=torch.int16, device=dev) for c in counts]
    for i, t in enumerate(coeffs):
        if not torch.is_tensor(t) or t.dtype != torch.int16 or t.device != dev or not t.is_contiguous() or t.numel() < counts[i]:
            raise L.EdgeStyleHipError(f"{what}: coefficients {i} must be a contiguous int16 device tensor of at least {counts[i]} values")
    if status is None:
        status = torch.empty((n,), dtype=torch.int32, device=dev)
    elif status.dtype != torch.int32 or status.device != dev or not status.is_contiguous() or status.numel() < n:
        raise L.EdgeStyleHipError(f"{what}: status must be a contiguous int32 device tensor of at least {n} values")
    need = int(lib.es_jpeg_entropy_decode_workspace_bytes(infos, n))
    if need == 0:
        L.check(-1, "es_jpeg_entropy_decode_workspace_bytes")
    workspace = _jpeg_bytes_buffer(what, workspace, need, dev, "workspace")
    fp = (C.c_void_p * n)(*[t.data_ptr() for t in files])
    fn = (C.c_size_t * n)(*[t.numel() for t in files])
    sp = (C.c_void_p * n)(*[t.data_ptr() for t in segments])
    tp = (C.c_void_p * n)(*[t.data_ptr() for t in tables])
    cp = (C.c_void_p * n)(*[t.data_ptr() for t in coeffs])
    L.check(lib.es_jpeg_entropy_decode(infos, n, fp, fn, sp, tp, int(subseq_bytes), cp, _ptr(status), _ptr(workspace), workspace.numel(), _stream()),
            "es_jpeg_entropy_decode")
    return coeffs, status


def jpeg_decode_dev_u8(datas: Sequence[bytes], infos, device, subseq_bytes: int = 0, out=None, status: Optional[torch.Tensor] = None,
                       staging_host: Optional[torch.Tensor] = None, staging_dev: Optional[torch.Tensor] = None,
                       workspace: Optional[torch.Tensor] = None):
    """es_jpeg_decode_dev_u8: parse + prepare on the host, one upload of the files, Huffman decoding and reconstruction on the device, up
    to 64 files (bytes objects; infos: their L.JpegInfo array) -> (a list of uint8 [H, W, 3] tensors on `device`, the int32 status
    tensor).  staging_host: a pinned uint8 host tensor the caller keeps untouched until the stream has passed the upload; when None one is
    allocated and the call waits for the stream before it returns.  The status is NOT read here (jpeg_status_check does)."""
    what = "jpeg_decode_dev_u8"
    n = len(datas)
    if n < 1 or len(infos) != n:
        raise L.EdgeStyleHipError(f"{what}: one info per file expected")
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    lib = L.load()
    ln = (C.c_size_t * n)(*[len(d) for d in datas])
    up = C.c_size_t(0)
    stage, need = int(lib.es_jpeg_decode_dev_staging_bytes(infos, ln, n, C.byref(up))), int(lib.es_jpeg_reconstruct_workspace_bytes(infos, n))
    if stage == 0 or need == 0:
        L.check(-1, "es_jpeg_decode_dev_staging_bytes")
    out, descs = _jpeg_outputs(what, infos, out, dev)
    own = staging_host is None
    if own:
        staging_host = torch.empty((up.value,), dtype=torch.uint8, pin_memory=True)
    elif staging_host.dtype != torch.uint8 or staging_host.is_cuda or not staging_host.is_contiguous() or staging_host.numel() < up.value:
        raise L.EdgeStyleHipError(f"{what}: staging_host must be a contiguous uint8 host tensor of at least {up.value} bytes")
    staging_dev = _jpeg_bytes_buffer(what, staging_dev, stage, dev, "staging_dev")
    workspace = _jpeg_bytes_buffer(what, workspace, need, dev, "workspace")
    if status is None:
        status = torch.empty((n,), dtype=torch.int32, device=dev)
    elif status.dtype != torch.int32 or status.device != dev or not status.is_contiguous() or status.numel() < n:
        raise L.EdgeStyleHipError(f"{what}: status must be a contiguous int32 device tensor of at least {n} values")
    bp = (C.c_void_p * n)(*[C.cast(C.c_char_p(d), C.c_void_p) for d in datas])
    L.check(lib.es_jpeg_decode_dev_u8(bp, ln, n, descs, int(subseq_bytes), _ptr(status), C.c_void_p(staging_host.data_ptr()), staging_host.numel(),
                                      _ptr(staging_dev), staging_dev.numel(), _ptr(workspace), workspace.numel(), _stream()), "es_jpeg_decode_dev_u8")
    if own:                                       # the upload reads the staging memory on the stream: it must not be freed before
        torch.cuda.current_stream().synchronize()
    return out, status


# ----------------------------------------------------------------------------------------------------------------
# JPEG encoding (csrc/jpeg_encode.hip): RGB or gray bytes -> the bytes of Pillow's file, written by the device.  edgestyle_amd/jpeg.py
# owns the convenient entry points (Pillow's argument spellings, the download); these take an L.JpegEncodeParams.
# ----------------------------------------------------------------------------------------------------------------
def jpeg_image_descs(what, images):
    """uint8 tensors or numpy arrays [H, W, 3] / [H, W] with dense pixels (rows may be pitched) -> the es_image_u8 array"""
    n = len(images)
    if n < 1:
        raise L.EdgeStyleHipError(f"{what}: no images")
    descs = (L.ImageU8 * n)()
    for i, t in enumerate(images):
        tensor = torch.is_tensor(t)
        shape = tuple(t.shape)
        stride = tuple(t.stride()) if tensor else tuple(t.strides)
        if ((t.dtype != torch.uint8 if tensor else str(t.dtype) != "uint8") or len(shape) not in (2, 3) or min(shape) < 1):
            raise L.EdgeStyleHipError(f"{what}: image {i} must be a uint8 [H, W, 3] or [H, W] array, got {shape}")
        ch = 1 if len(shape) == 2 else shape[2]
        if ((shape[1] > 1 and stride[1] != ch) or (len(shape) == 3 and ch > 1 and stride[2] != 1)
                or (shape[0] > 1 and stride[0] < shape[1] * ch)):      # (the stride of an axis of one element says nothing)
            raise L.EdgeStyleHipError(f"{what}: image {i} must have dense pixels (rows may be pitched), got strides {stride}")
        descs[i].data = t.data_ptr() if tensor else t.ctypes.data
        descs[i].height, descs[i].width, descs[i].channels = shape[0], shape[1], ch
        descs[i].row_stride = stride[0] if shape[0] > 1 else shape[1] * ch
    return descs


def jpeg_encode_infos(what, descs, params):
    lib = L.load()
    infos = (L.JpegInfo * len(descs))()
    for i, d in enumerate(descs):
        L.check(lib.es_jpeg_encode_info_host(d.width, d.height, d.channels, C.byref(params), C.byref(infos[i])), "es_jpeg_encode_info_host")
    return infos


def _jpeg_encode_buffers(what, infos, params, dev, out, lengths, workspace):
    lib = L.load()
    n = len(infos)
    caps = []
    for i in range(n):
        caps.append(int(lib.es_jpeg_encode_capacity(C.byref(infos[i]), C.byref(params))))
        if caps[-1] == 0:
            L.check(-1, "es_jpeg_encode_capacity")
    need = int(lib.es_jpeg_encode_workspace_bytes(infos, n, C.byref(params)))
    if need == 0:
        L.check(-1, "es_jpeg_encode_workspace_bytes")
    if out is None:
        out = [torch.empty((c,), dtype=torch.uint8, device=dev) for c in caps]
    if len(out) != n or any(o.dtype != torch.uint8 or o.device != dev or not o.is_contiguous() for o in out):
        raise L.EdgeStyleHipError(f"{what}: {n} contiguous uint8 output tensors on {dev} expected")
    if lengths is None:
        lengths = torch.empty((n,), dtype=torch.uint32, device=dev)
    if lengths.dtype != torch.uint32 or lengths.device != dev or not lengths.is_contiguous() or lengths.numel() < n:
        raise L.EdgeStyleHipError(f"{what}: lengths must be a contiguous uint32 tensor of {n} values on {dev}")
    workspace = _jpeg_bytes_buffer(what, workspace, need, dev, "workspace")
    op = (C.c_void_p * n)(*[o.data_ptr() for o in out])
    cp = (C.c_size_t * n)(*[o.numel() for o in out])
    return out, lengths, workspace, op, cp


def jpeg_forward(images: Sequence[torch.Tensor], params, coeffs=None):
    """es_jpeg_forward: device uint8 images -> (infos, a list of int16 coefficient tensors in the decoder's layout).  One launch per 16."""
    what = "jpeg_forward"
    descs = jpeg_image_descs(what, images)
    infos = jpeg_encode_infos(what, descs, params)
    dev = images[0].device
    lib = L.load()
    n = len(images)
    counts = [int(lib.es_jpeg_coeff_count(C.byref(infos[i]))) for i in range(n)]
    if coeffs is None:
        coeffs = [torch.empty((c,), dtype=torch.int16, device=dev) for c in counts]
    if len(coeffs) != n or any(t.dtype != torch.int16 or t.device != dev or not t.is_contiguous() or t.numel() < c for t, c in zip(coeffs, counts)):
        raise L.EdgeStyleHipError(f"{what}: one contiguous int16 coefficient tensor per image on {dev} expected")
    if any(not t.is_cuda or t.device != dev for t in images):
        raise L.EdgeStyleHipError(f"{what}: the images must be on one device")
    cp = (C.c_void_p * n)(*[t.data_ptr() for t in coeffs])
    L.check(lib.es_jpeg_forward(descs, n, C.byref(params), cp, None, 0, _stream()), "es_jpeg_forward")
    return infos, coeffs


def jpeg_entropy_encode(infos, params, coeffs: Sequence[torch.Tensor], out=None, lengths=None, workspace=None):
    """es_jpeg_entropy_encode: coefficient tensors -> (uint8 buffers holding the whole files, uint32 lengths), all on the device; nothing
    is read back.  7 launches per 16 images."""
    what = "jpeg_entropy_encode"
    n = len(infos)
    if n < 1 or len(coeffs) != n:
        raise L.EdgeStyleHipError(f"{what}: one coefficient tensor per image expected")
    dev = coeffs[0].device
    lib = L.load()
    for i, t in enumerate(coeffs):
        if not torch.is_tensor(t) or t.dtype != torch.int16 or t.device != dev or not t.is_cuda or not t.is_contiguous() \
                or t.numel() < int(lib.es_jpeg_coeff_count(C.byref(infos[i]))):
            raise L.EdgeStyleHipError(f"{what}: coefficients {i} must be a contiguous int16 device tensor of es_jpeg_coeff_count values")
    out, lengths, workspace, op, cap = _jpeg_encode_buffers(what, infos, params, dev, out, lengths, workspace)
    cp = (C.c_void_p * n)(*[t.data_ptr() for t in coeffs])
    L.check(lib.es_jpeg_entropy_encode(infos, n, C.byref(params), cp, op, cap, _ptr(lengths), _ptr(workspace), workspace.numel(), _stream()),
            "es_jpeg_entropy_encode")
    return out, lengths


def jpeg_encode_u8(images: Sequence[torch.Tensor], params, out=None, lengths=None, workspace=None):
    """es_jpeg_encode_u8: up to 64 device uint8 images -> (uint8 buffers holding the files, uint32 lengths) on the device; nothing is read
    back and nothing synchronises.  8 launches per 16 images."""
    what = "jpeg_encode_u8"
    descs = jpeg_image_descs(what, images)
    dev = images[0].device
    if any(not torch.is_tensor(t) or not t.is_cuda or t.device != dev for t in images):
        raise L.EdgeStyleHipError(f"{what}: the images must be tensors on one device")
    infos = jpeg_encode_infos(what, descs, params)
    n = len(images)
    out, lengths, workspace, op, cap = _jpeg_encode_buffers(what, infos, params, dev, out, lengths, workspace)
    L.check(L.load().es_jpeg_encode_u8(descs, n, C.byref(params), op, cap, _ptr(lengths), _ptr(workspace), workspace.numel(), _stream()),
            "es_jpeg_encode_u8")
    return out, lengths


# ----------------------------------------------------------------------------------------------------------------
# mask post-processing (csrc/mask.hip): bit-packed morphology, largest 8-connected component, boolean algebra, draw_binary_mask
# and create_sam_images in one call.  Masks are uint8 (or bool) device tensors [count, H, W]; results are uint8 of 0 / 1.
# ----------------------------------------------------------------------------------------------------------------
def _mask_operand(t: torch.Tensor, what: str, shape=None) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype not in (torch.uint8, torch.bool) or not t.is_cuda:
        raise L.EdgeStyleHipError(f"{what}: a mask must be a uint8 or bool device tensor")
    if t.dim() != 3 or min(t.shape) < 1 or not t.is_contiguous():
        raise L.EdgeStyleHipError(f"{what}: a mask must be a dense [count, H, W] tensor, got {tuple(t.shape)} with strides {t.stride()}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise L.EdgeStyleHipError(f"{what}: masks of one call must have one shape ({tuple(t.shape)} vs {tuple(shape)})")
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _mask_out(out: Optional[torch.Tensor], shape, dev, what: str) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=dev)
    if out.dtype != torch.uint8 or out.device != dev or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise L.EdgeStyleHipError(f"{what}: out must be a contiguous uint8 {tuple(shape)} tensor on {dev}")
    return out


def mask_workspace_bytes(H: int, W: int, count: int) -> int:
    need = int(L.load().es_mask_workspace_bytes(int(H), int(W), int(count)))
    if need == 0:
        L.check(-1, "es_mask_workspace_bytes")
    return need


def _mask_workspace(workspace: Optional[torch.Tensor], H: int, W: int, count: int, dev, what: str) -> torch.Tensor:
    if workspace is None:
        return torch.empty((mask_workspace_bytes(H, W, count),), dtype=torch.uint8, device=dev)
    if workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
        raise L.EdgeStyleHipError(f"{what}: workspace must be a contiguous uint8 tensor on {dev}")
    return workspace


def mask_morph(mask: torch.Tensor, radii: Sequence[int], out: Optional[torch.Tensor] = None,
               workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The chain of clipped-window dilations (r > 0) and erosions (r < 0) `radii`, in order, on [count, H, W]; out may be mask."""
    m = _mask_operand(mask, "mask_morph")
    n, H, W = m.shape
    out = _mask_out(out, m.shape, m.device, "mask_morph")
    ws = _mask_workspace(workspace, H, W, n, m.device, "mask_morph")
    arr = (C.c_int32 * max(len(radii), 1))(*[int(r) for r in radii])
    L.check(L.load().es_mask_morph(_ptr(m), _ptr(out), n, H, W, arr, len(radii), _ptr(ws), ws.numel(), _stream()), "es_mask_morph")
    return out


def mask_largest_component(mask: torch.Tensor, out: Optional[torch.Tensor] = None, area_out: Optional[torch.Tensor] = None,
                           workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The largest 8-connected component of each mask (ties: the one that starts first in row-major order; no true pixel: all
    true, as the reference's labeled_array == 0).  area_out: int32 [count] device tensor that receives the winners' areas."""
    m = _mask_operand(mask, "mask_largest_component")
    n, H, W = m.shape
    out = _mask_out(out, m.shape, m.device, "mask_largest_component")
    if area_out is not None and (area_out.dtype != torch.int32 or area_out.device != m.device or tuple(area_out.shape) != (n,)
                                 or not area_out.is_contiguous()):
        raise L.EdgeStyleHipError(f"mask_largest_component: area_out must be a contiguous int32 [{n}] tensor on {m.device}")
    ws = _mask_workspace(workspace, H, W, n, m.device, "mask_largest_component")
    L.check(L.load().es_mask_largest_component(_ptr(m), _ptr(out), _ptr(area_out), n, H, W, _ptr(ws), ws.numel(), _stream()),
            "es_mask_largest_component")
    return out


def mask_logic(a: torch.Tensor, b: torch.Tensor, op: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a op b for op in L.MASK_AND | L.MASK_OR | L.MASK_ANDNOT (a & ~b); out may be a or b."""
    a = _mask_operand(a, "mask_logic")
    b = _mask_operand(b, "mask_logic", a.shape)
    out = _mask_out(out, a.shape, a.device, "mask_logic")
    L.check(L.load().es_mask_logic(_ptr(a), _ptr(b), _ptr(out), a.numel(), int(op), _stream()), "es_mask_logic")
    return out


def image_mask_fill_u8(images: Optional[Sequence[torch.Tensor]], mask: torch.Tensor, colour, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """draw_binary_mask for count images: [count, H, W, 3] that keeps images[i] where mask[i] is true and is `colour` elsewhere;
    images None: images of zeros."""
    m = _mask_operand(mask, "image_mask_fill_u8")
    n, H, W = m.shape
    descs = None
    if images is not None:
        if len(images) != n:
            raise L.EdgeStyleHipError(f"image_mask_fill_u8: {len(images)} images for {n} masks")
        descs = image_descriptors(images, "image_mask_fill_u8")
    out = _mask_out(out, (n, H, W, 3), m.device, "image_mask_fill_u8")
    col = (C.c_uint8 * 3)(*[int(c) for c in colour])
    L.check(L.load().es_image_mask_fill_u8(descs, _ptr(m), _ptr(out), n, H, W, col, _stream()), "es_image_mask_fill_u8")
    return out


def sam_compose(images: Optional[Sequence[torch.Tensor]], subject: torch.Tensor, body: torch.Tensor, clothes: torch.Tensor,
                head: torch.Tensor, want_masks: bool = True, want_images: bool = True, masks_out: Optional[torch.Tensor] = None,
                images_out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """create_sam_images after the networks, one call: -> (masks [count, 4, H, W]: all, agnostic, clothes, head | None,
    images [count, 5, H, W, 3]: subject, mask, agnostic, clothes, head | None)."""
    s = _mask_operand(subject, "sam_compose")
    b, c, h = (_mask_operand(t, "sam_compose", s.shape) for t in (body, clothes, head))
    n, H, W = s.shape
    descs = None
    if want_images:
        if images is None or len(images) != n:
            raise L.EdgeStyleHipError(f"sam_compose: {n} images are needed for {n} sets of masks")
        descs = image_descriptors(images, "sam_compose")
    masks_out = _mask_out(masks_out, (n, 4, H, W), s.device, "sam_compose") if want_masks else None
    images_out = _mask_out(images_out, (n, 5, H, W, 3), s.device, "sam_compose") if want_images else None
    ws = _mask_workspace(workspace, H, W, n, s.device, "sam_compose")
    L.check(L.load().es_sam_compose(descs, _ptr(s), _ptr(b), _ptr(c), _ptr(h), n, H, W, _ptr(masks_out), _ptr(images_out), _ptr(ws),
                                    ws.numel(), _stream()), "es_sam_compose")
    return masks_out, images_out


# ----------------------------------------------------------------------------------------------------------------
# seeded noise: torch's device Philox stream restated (csrc/rng.hip)
_ROUND = {None: L.ES_F32, torch.float32: L.ES_F32, torch.float16: L.ES_F16, torch.bfloat16: L.ES_BF16}


def philox_blocks(numel: int, device=None) -> int:
    """The grid torch's generator kernel takes for a draw of `numel` floats on `device` (it decides layout and advance)."""
    lib = L.load()
    dev = torch.device("cuda" if device is None else device)
    cap = lib.es_philox_block_cap(torch.cuda.current_device() if dev.index is None else dev.index)
    if cap < 1:
        L.check(cap, "es_philox_block_cap")
    return lib.es_philox_blocks(numel, cap)


def randn(shape, seed: int, offset: int, *, blocks: int = 0, scale: float = 1.0, round_dtype=None, nhwc=None,
          device=None, out: Optional[torch.Tensor] = None):
    """torch.randn(shape, device=device, generator=g) for a device generator g with initial_seed() == seed and get_offset() ==
    offset, as fp32, and the offset g has afterwards: (tensor, advanced offset).

    blocks: torch's grid for the draw, 0 = this device's (philox_blocks).  round_dtype: None | torch.float16 | torch.bfloat16 -
    the values of a draw in that dtype, widened to fp32.  scale multiplies the result after that rounding.  nhwc: None = the
    tensor has `shape`; True or a channel stride >= C = shape is [N, C, ...], drawn in that order and returned as
    [N, ..., stride] (channels-last; channels C.. of a padded result are zero, or keep what `out` held)."""
    lib = L.load()
    shape = tuple(int(v) for v in shape)
    numel = math.prod(shape)
    if round_dtype not in _ROUND:
        raise L.EdgeStyleHipError(f"randn: round_dtype must be None, torch.float16 or torch.bfloat16, not {round_dtype}")
    dev = torch.device("cuda" if device is None else device) if out is None else out.device
    if dev.type != "cuda":
        raise L.EdgeStyleHipError(f"randn: draws on the GPU, not on {dev} (lib.es_randn_host is the CPU form)")
    d = L.RandnDesc(seed=int(seed) & (2 ** 64 - 1), offset=int(offset), numel=numel, blocks=int(blocks), scale=float(scale),
                    round_dtype=_ROUND[round_dtype])
    out_shape = shape
    if nhwc is not None and nhwc is not False:
        if len(shape) < 3:
            raise L.EdgeStyleHipError(f"randn: nhwc needs a shape [N, C, ...], got {shape}")
        d.N, d.C, d.HW = shape[0], shape[1], math.prod(shape[2:])
        d.Cstride = shape[1] if nhwc is True else int(nhwc)
        out_shape = (shape[0],) + shape[2:] + (int(d.Cstride),)
    with torch.cuda.device(dev):
        if not d.blocks:
            d.blocks = philox_blocks(max(numel, 1), dev)
        if out is None:
            out = (torch.zeros if d.Cstride > d.C else torch.empty)(out_shape, dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or tuple(out.shape) != out_shape or not out.is_contiguous():
            raise L.EdgeStyleHipError(f"randn: out must be a contiguous fp32 {out_shape} tensor")
        L.check(lib.es_randn(_ptr(out), C.byref(d), _stream()), "es_randn")
    return out, int(offset) + lib.es_philox_advance(numel, d.blocks)
