"""CPU suite: host logic of the product package (no GPU, no compute calls): C-ABI surface, weight packing,
on-disk layout round trips, reference error behaviour, scheduler tables, sharding."""
import ctypes
import os
import re

import pytest
import torch

from edgestyle_amd import config as C, weights as W, ops, lib
from edgestyle_amd.models import (UNet2DConditionModel, ControlNetModel, ControlLoRAModel, FusedControlLoRAModel,
                                  AutoencoderKL, EdgeStyleMultiControlNetModel, unet_config_from_json)
from edgestyle_amd.schedulers import DDIMScheduler
from edgestyle_amd.dist import shard_range, shard_seed
from tests.helpers import make_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cabi_library_loads_and_exports_every_declared_symbol():
    assert os.path.exists(lib.LIB_PATH), "build with __graft_entry__.build()"
    header = open(os.path.join(ROOT, "include", "edgestyle_hip.h")).read()
    declared = set(re.findall(r"\b(es_[a-z0-9_]+)\s*\(", header))
    declared = {d for d in declared if not d.endswith("_desc") or d == "es_sizeof_desc"}
    declared -= {"es_ctx_geometry"}
    assert declared == set(lib.SYMBOLS), declared ^ set(lib.SYMBOLS)
    h = ctypes.CDLL(lib.LIB_PATH)
    for name in declared:
        assert getattr(h, name) is not None
    L = lib.load()
    assert L.es_abi_version() == 7
    # struct layouts agree with the C side (sizes are what the kernels index with)
    for i, st in enumerate((lib.GemmDesc, lib.AttnDesc, lib.GnDesc, lib.FusionDesc, lib.LnDesc, lib.XsDesc)):
        assert L.es_sizeof_desc(i) == ctypes.sizeof(st)


def test_plan_records_nothing_and_launches_nothing_without_a_gpu():
    """es_plan object life cycle on the host (no compute calls): create / begin / end / size / destroy; a second plan
    cannot start recording while one records."""
    L = lib.load()
    a, b = ctypes.c_void_p(L.es_plan_create()), ctypes.c_void_p(L.es_plan_create())
    assert L.es_plan_size(a) == 0
    assert L.es_plan_begin_record(a) == 0
    assert L.es_plan_begin_record(b) != 0 and b"recording" in L.es_last_error()
    assert L.es_plan_end_record(b) != 0
    assert L.es_plan_end_record(a) == 0 and L.es_plan_size(a) == 0
    ctx = ctypes.c_void_p()
    assert L.es_ctx_create(0, ctypes.byref(ctx)) == 0
    assert L.es_ctx_plan_size(ctx, lib.PLAN_STEP) == -1
    assert L.es_ctx_set_plan(ctx, lib.PLAN_STEP, a) == 0 and L.es_ctx_plan_size(ctx, lib.PLAN_STEP) == 0
    geo = lib.CtxGeometry(B=1, cfg=1, h=8, w=8, latent_channels=4, latent_pad=8, n_conds=7, n_steps=4, dtype=0)
    assert L.es_ctx_set_geometry(ctx, ctypes.byref(geo)) != 0            # 7 conditions: refused
    L.es_ctx_destroy(ctx)                                               # destroys plan a
    L.es_plan_destroy(b)


def test_plan_image_round_trip_markers_and_context_image_errors(tmp_path):
    """Host-only parts of the context-image machinery: es_plan_import / es_plan_export round trip of a hand-made launch
    list, refusal of truncated or inconsistent images, and es_ctx_load's errors on a missing / foreign file (nothing touches
    a GPU: the file is rejected before any HIP call)."""
    import struct
    L = lib.load()
    # a hand-made image of two recorded calls (csrc/plan.h: 18 = es_memcpy {dst, src, bytes}, 16 = es_incr {ctr}); nothing
    # can RECORD on a CPU-only host (every entry point validates and launches), but import / export are host-only
    blob = struct.pack("<QQQ", 0x1000, 0x2000, 64) + b"\0" * 8 + struct.pack("<Q", 0x3000)
    img = struct.pack("<QQ", 2, len(blob)) + struct.pack("<qQQ", 18, 0, 24) + struct.pack("<qQQ", 16, 32, 8) + blob
    buf = (ctypes.c_char * len(img)).from_buffer_copy(img)
    q = ctypes.c_void_p(L.es_plan_import(buf, len(img)))
    assert q.value and L.es_plan_size(q) == 2 and L.es_plan_count(q, 18) == 1 and L.es_plan_count(q, 16) == 1
    n = L.es_plan_export(q, None, 0)
    assert n == len(img)
    out = (ctypes.c_char * n)()
    assert L.es_plan_export(q, out, n) == n and bytes(out) == img
    assert not L.es_plan_import(buf, len(img) - 8) and b"truncated" in L.es_last_error()
    bad_op = struct.pack("<QQ", 1, 8) + struct.pack("<qQQ", 16, 4, 8) + b"\0" * 8          # record runs past the blob
    assert not L.es_plan_import((ctypes.c_char * len(bad_op)).from_buffer_copy(bad_op), len(bad_op))
    L.es_plan_destroy(q)
    ctx = ctypes.c_void_p()
    assert L.es_ctx_load(str(tmp_path / "missing.esctx").encode(), 0, ctypes.byref(ctx)) != 0 and b"open" in L.es_last_error()
    bad = tmp_path / "bad.esctx"
    bad.write_bytes(b"not a context image at all, just some bytes" * 4)
    assert L.es_ctx_load(str(bad).encode(), 0, ctypes.byref(ctx)) != 0 and b"not a context image" in L.es_last_error()


# ----------------------------------------------------------------------------------------------------------------
# es_ctx_save_ranges, the one writer of a context image, on a host without a GPU: a context assembled from hand-made plans
# and invented addresses.  With path NULL, or with an image that has no data extents, nothing dereferences them.
# The memory map of these tests (S = allocator segment; S2 is used by nobody; 64 KiB = 0x10000):
#   S0 0x10000 + 0x20001   -> arena 0x00000 (slot 0x20100: rounded up to 256)
#   S1 0x30001 + 0x00100   -> arena 0x20100 (adjacent: S0's end is S1's first byte)
#   S2 0x40000 + 0x01000   -> no slot
#   S3 0x50000 + 0x40000   -> arena 0x20200; the arena is 0x60200 bytes
# ----------------------------------------------------------------------------------------------------------------
_SEGS = [(0x50000, 0x40000), (0x10000, 0x20001), (0x40000, 0x1000), (0x30001, 0x100)]        # handed over unsorted
_ARENA_OF = {0x10000: 0x0, 0x10008: 0x8, 0x10010: 0x10, 0x30000: 0x20000,                    # S0 (0x30000: its last byte)
             0x30001: 0x20100, 0x30100: 0x201FF,                                              # S1: first and last byte
             0x50000: 0x20200, 0x50010: 0x20210, 0x50020: 0x20220, 0x50040: 0x20240, 0x50100: 0x20300,
             0x60001: 0x30201, 0x60002: 0x30202, 0x60010: 0x30210, 0x70002: 0x40202}                            # S3


def _image_plans(at):
    """The two plans of these tests as {which: (plan image, [blob positions of the non-null pointer fields, in call order])};
    `at` maps an address to what the image is to hold in its place."""
    import struct
    F = lib.FusionDesc
    step = (struct.pack("<QQQ", at(0x50000), at(0x10000), 64)            # @0   es_memcpy {dst, src, bytes}
            + struct.pack("<Q", at(0x30000))                             # @24  es_incr {ctr}
            + struct.pack("<QQQii", at(0x30001), 0, at(0x60001), 5, 3)   # @32  es_gather_row {table, idx (null), out, row_len, nrows}
            + struct.pack("<QQQ", at(0x50010), at(0x60002), 8)           # @64  es_memcpy
            + struct.pack("<QQQ", at(0x50020), at(0x70002), 8))          # @88  es_memcpy
    step_ops = [(18, 0, 24), (16, 24, 8), (17, 32, 32), (18, 64, 24), (18, 88, 24)]
    a, b = F(), F()                                                       # es_fusion_blocks: two elements in one record
    a.res[0], a.w1, a.out, a.C = at(0x30100), at(0x10008), at(0x50100), 320
    b.res[5], b.u, b.HW = at(0x10010), at(0x60010), 64
    sz = ctypes.sizeof(F)
    out = {}
    for which, ops_, blob, pos in ((lib.PLAN_STEP, step_ops, step, [0, 8, 24, 32, 48, 64, 72, 88, 96]),
                                   (lib.PLAN_DECODE, [(8, 0, 2 * sz)], bytes(a) + bytes(b),
                                    [F.res.offset, F.w1.offset, F.out.offset, sz + F.res.offset + 40, sz + F.u.offset])):
        out[which] = (struct.pack("<QQ", len(ops_), len(blob)) + b"".join(struct.pack("<qQQ", *o) for o in ops_) + blob, pos)
    return out


def _image_ctx(L, plans, binds=()):
    ctx = ctypes.c_void_p()
    assert L.es_ctx_create(0, ctypes.byref(ctx)) == 0
    for which, img in plans.items():
        p = ctypes.c_void_p(L.es_plan_import((ctypes.c_char * len(img)).from_buffer_copy(img), len(img)))
        assert p.value and L.es_ctx_set_plan(ctx, which, p) == 0
    for slot, addr, nbytes in binds:
        assert L.es_ctx_bind(ctx, slot, ctypes.c_void_p(addr), nbytes) == 0
    return ctx


def _ranges(r):
    return (lib.MemRange * len(r))(*r), len(r)


_BINDS = ((lib.BUF_SAMPLE, 0x70002, 16), (lib.BUF_IMAGE, 0x50040, 32))


def test_context_image_layout_segments_extents_and_relocation_counts():
    """Layout phase alone (path NULL): which segments get an arena slot, how large the arena is, which blocks travel as data
    and how many pointer fields of each plan are relocated - against figures worked out by hand from the map above."""
    L = lib.load()
    ctx = _image_ctx(L, {w: img for w, (img, _) in _image_plans(lambda a: a).items()}, _BINDS)
    blocks = [(0x10000, 0x10001),      # A: 64 KiB + 1, only read (memcpy src, fusion w1 and res)              -> data
              (0x20001, 0x10000),      # B: 64 KiB, written (es_incr reads and writes it): small                 -> data
              # S1 has no block: 0x30001 and 0x30100 are relocated and add nothing
              (0x50000, 0x10001),      # C: 64 KiB + 1, only written (a bound slot lies in it, too)             -> space
              (0x60001, 0x10001),      # D: 64 KiB + 1, written by es_gather_row, read by an es_memcpy (+ fusion u) -> space
              (0x70002, 0x10001),      # E: 64 KiB + 1, only read by the plans, but ES_BUF_SAMPLE is bound here -> space
              (0x80003, 0x100)]        # F: referenced by nobody                                                -> nothing
    info = lib.CtxImageInfo()
    assert L.es_ctx_save_ranges(ctx, None, *_ranges(_SEGS), *_ranges(blocks[::-1]), ctypes.byref(info)) == 0, L.es_last_error()
    assert (info.segments, info.arena_bytes) == (3, 0x60200)
    assert (info.extents, info.data_bytes) == (2, 0x10001 + 0x10000)
    assert list(info.relocations) == [0, 0, 9, 5, 0, 0]            # null fields (es_gather_row's idx, most of a fusion element) skipped
    # without ES_BUF_SAMPLE in it, E is only read: a third extent
    ctx2 = _image_ctx(L, {w: img for w, (img, _) in _image_plans(lambda a: a).items()}, _BINDS[1:])
    assert L.es_ctx_save_ranges(ctx2, None, *_ranges(_SEGS), *_ranges(blocks), ctypes.byref(info)) == 0
    assert (info.extents, info.data_bytes, info.arena_bytes) == (3, 0x10001 + 0x10000 + 0x10001, 0x60200)
    # no block table: only what the context's builder recorded as data travels - nothing, for a context assembled by hand
    assert L.es_ctx_save_ranges(ctx, None, *_ranges(_SEGS), None, 0, ctypes.byref(info)) == 0
    assert (info.segments, info.arena_bytes, info.extents, info.data_bytes) == (3, 0x60200, 0, 0) and list(info.relocations) == [0, 0, 9, 5, 0, 0]
    # a context that uses S0 alone: one slot, rounded up to 256
    ctx3 = _image_ctx(L, {lib.PLAN_PREP: _pointer_plan([(16, 0x10000)])})
    assert L.es_ctx_save_ranges(ctx3, None, *_ranges(_SEGS), None, 0, ctypes.byref(info)) == 0
    assert (info.segments, info.arena_bytes) == (1, 0x20100) and list(info.relocations) == [0, 1, 0, 0, 0, 0]
    for c in (ctx, ctx2, ctx3):
        L.es_ctx_destroy(c)


def _pointer_plan(calls):
    """a plan image of one-pointer calls [(kind, address)] (es_incr = 16 {ctr})"""
    import struct
    return (struct.pack("<QQ", len(calls), 8 * len(calls)) + b"".join(struct.pack("<qQQ", k, 8 * i, 8) for i, (k, _) in enumerate(calls))
            + b"".join(struct.pack("<Q", a) for _, a in calls))


def test_context_image_refusals_name_the_cause_and_leave_no_file(tmp_path):
    import struct
    L = lib.load()
    path = tmp_path / "no.esctx"

    def refused(ctx, segs, *words):
        info = lib.CtxImageInfo()
        for p in (None, str(path).encode()):                     # the same verdict with and without a file to write
            assert L.es_ctx_save_ranges(ctx, p, *_ranges(segs), None, 0, ctypes.byref(info)) != 0
            err = L.es_last_error().decode()
            assert all(w in err for w in words), err
            assert not path.exists() and not (tmp_path / "no.esctx.tmp").exists()
        L.es_ctx_destroy(ctx)

    # S1's end belongs to nobody (S2 begins later); S0's end is S1's first byte and is fine (the layout test relocates it)
    refused(_image_ctx(L, {lib.PLAN_STEP: _pointer_plan([(16, 0x10000), (16, 0x30101)])}), _SEGS, "op kind 16", "0x30101", "outside every segment")
    refused(_image_ctx(L, {lib.PLAN_STEP: _pointer_plan([(16, 0x30001)])}), [(0x10000, 0x20001), (0x30002, 0x100)], "op kind 16", "0x30001")
    refused(_image_ctx(L, {}, [(lib.BUF_EHS, 0x41000, 8)]), _SEGS, "bound slot 2", "0x41000", "outside every segment")
    refused(_image_ctx(L, {}, [(lib.BUF_EHS, 0x30100, 2)]), _SEGS, "bound slot 2", "outside every segment")       # runs past S1's last byte
    refused(_image_ctx(L, {lib.PLAN_STEP: _pointer_plan([(16, 0x10000)])}), _SEGS + [(0x30000, 0x10)], "overlapping segments")
    refused(_image_ctx(L, {lib.PLAN_STEP: _pointer_plan([(16, 0x10000)])}), [(0x10000, 0)], "empty")
    # es_gather_row {table, idx, out, ...} recorded with 16 bytes: its third pointer field would lie behind the record
    short = struct.pack("<QQ", 1, 16) + struct.pack("<qQQ", 17, 0, 16) + struct.pack("<QQ", 0x10000, 0x10008)
    refused(_image_ctx(L, {lib.PLAN_STEP: short}), _SEGS, "pointer field lies outside its record")
    # es_ctx_save is the same writer with the context's own arena as the one segment: a context without one is sent here
    ctx = _image_ctx(L, {lib.PLAN_STEP: _pointer_plan([(16, 0x10000)])})
    assert L.es_ctx_save(ctx, str(path).encode()) != 0
    assert b"does not own a device arena" in L.es_last_error() and b"es_ctx_save_ranges" in L.es_last_error() and not path.exists()
    L.es_ctx_destroy(ctx)


def test_context_image_without_data_extents_byte_for_byte(tmp_path):
    """An image whose referenced blocks are all large and written has no data, so writing it touches no GPU: the whole file
    against one assembled here - magic and format 3, ABI 7, geometry, options, an odd fp32 schedule padded to 8 bytes, the f64
    schedule, the block table of the used segments, per plan `size | image with arena offsets in the blob | n_rel | (position,
    offset)` with a zero size for an absent plan, the slot table with -1 for unbound slots, zero extents."""
    import struct
    L = lib.load()
    ctx = _image_ctx(L, {w: img for w, (img, _) in _image_plans(lambda a: a).items()}, _BINDS)
    geo = lib.CtxGeometry(B=1, cfg=1, h=8, w=8, latent_channels=4, latent_pad=8, n_conds=6, n_steps=4, dtype=lib.ES_F16, guess_mode=0)
    assert L.es_ctx_set_geometry(ctx, ctypes.byref(geo)) == 0
    scales = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    assert L.es_ctx_set_options(ctx, (ctypes.c_float * 6)(*scales), 0.25, 0.75, 2) == 0
    ac, ac64 = [0.75, 0.5, 0.25], [0.875, 0.125]
    assert L.es_ctx_set_alphas_cumprod(ctx, (ctypes.c_float * 3)(*ac), 3) == 0
    assert L.es_ctx_set_alphas_cumprod_f64(ctx, (ctypes.c_double * 2)(*ac64), 2) == 0
    blocks = [(0x10000, 0x20001), (0x50000, 0x40000)]              # S0 and S3 as one block each, both written; S1 without a block
    path = tmp_path / "ctx.esctx"
    info = lib.CtxImageInfo()
    assert L.es_ctx_save_ranges(ctx, str(path).encode(), *_ranges(_SEGS), *_ranges(blocks), ctypes.byref(info)) == 0, L.es_last_error()
    assert (info.segments, info.arena_bytes, info.extents, info.data_bytes) == (3, 0x60200, 0, 0)
    want = b"ESCTX\x03\x00\x00" + struct.pack("<IIQ", 7, 3, 0x60200) + bytes(geo)
    want += struct.pack("<6fffiIiI", *scales, 0.25, 0.75, 2, 3, lib.SCHED_DDIM, 2)
    want += struct.pack("<3f4x2d", *ac, *ac64)
    want += struct.pack("<QQQQQQ", 0x0, 0x20001, 0x20100, 0x100, 0x20200, 0x40000)
    given, moved = _image_plans(lambda a: a), _image_plans(_ARENA_OF.__getitem__)
    for which in range(lib.PLAN_COUNT):
        if which not in moved:
            want += struct.pack("<Q", 0)
            continue
        img, pos = moved[which]
        blob0 = len(img) - struct.unpack("<Q", img[8:16])[0]
        want += struct.pack("<Q", len(img)) + img + struct.pack("<Q", len(pos))
        for p in pos:
            addr = struct.unpack("<Q", given[which][0][blob0 + p:blob0 + p + 8])[0]
            want += struct.pack("<QQ", p, _ARENA_OF[addr])
    slots = {lib.BUF_SAMPLE: (0x40202, 16), lib.BUF_IMAGE: (0x20240, 32)}
    for slot in range(lib.BUF_COUNT):
        want += struct.pack("<qQ", *slots.get(slot, (-1, 0)))
    want += struct.pack("<Q", 0)
    got = path.read_bytes()
    assert got == want, next(i for i, (x, y) in enumerate(zip(got, want)) if x != y) if len(got) == len(want) else (len(got), len(want))
    assert not (tmp_path / "ctx.esctx.tmp").exists()
    # the same context saves to the same bytes, in whatever order the segments are handed over
    assert L.es_ctx_save_ranges(ctx, str(path).encode(), *_ranges(_SEGS[::-1]), *_ranges(blocks), None) == 0 and path.read_bytes() == want
    L.es_ctx_destroy(ctx)


def test_native_ddim_coefficients_match_the_host_scheduler():
    """es_ddim_coef_table (what es_denoise_loop derives from `timesteps`, host-only code) vs DDIMScheduler.coef_table():
    bit for bit with the scheduler's alphas_cumprod handed over, within 1e-6 with the library's own SD1.5 schedule."""
    import numpy as np
    L = lib.load()
    fp = ctypes.POINTER(ctypes.c_float)
    for T in (4, 20, 50):
        s = DDIMScheduler()
        ts = s.set_timesteps(T).float().numpy().astype(np.float32)
        want = s.coef_table().numpy()
        ac = s.alphas_cumprod.numpy().astype(np.float32)
        out = np.zeros((T, 4), dtype=np.float32)
        assert L.es_ddim_coef_table(ac.ctypes.data_as(fp), len(ac), ts.ctypes.data_as(fp), T, out.ctypes.data_as(fp)) == 0
        assert np.array_equal(out, want)
        assert L.es_ddim_coef_table(None, 0, ts.ctypes.data_as(fp), T, out.ctypes.data_as(fp)) == 0
        assert np.abs(out - want).max() < 1e-6


def test_native_unipc_coefficients_match_the_host_scheduler_bitwise():
    """es_unipc_coef_table (what es_denoise_loop derives from `timesteps` under ES_SCHED_UNIPC; csrc/plan.hip) ==
    UniPCMultistepScheduler.coef_table(), with the library's own double-precision SD1.5 schedule and with the scheduler's."""
    import numpy as np
    from edgestyle_amd.schedulers import UniPCMultistepScheduler
    L = lib.load()
    fp = ctypes.POINTER(ctypes.c_float)
    for T in (2, 3, 4, 20, 50):
        s = UniPCMultistepScheduler()
        ts = s.set_timesteps(T).float().numpy().astype(np.float32)
        want = s.coef_table().numpy()
        out = np.zeros((T, 12), dtype=np.float32)
        assert L.es_unipc_coef_table(None, 0, ts.ctypes.data_as(fp), T, out.ctypes.data_as(fp)) == 0
        assert np.array_equal(out, want)
        ac = s.alphas_cumprod.numpy().astype(np.float64)
        assert L.es_unipc_coef_table(ac.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(ac), ts.ctypes.data_as(fp), T, out.ctypes.data_as(fp)) == 0
        assert np.array_equal(out, want)


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", "/nonexistent/libedgestyle_hip.so")
    with pytest.raises(lib.EdgeStyleHipError):
        lib.load()


def test_cpu_device_is_refused_not_emulated():
    ucfg = C.tiny_unet()
    unet = UNet2DConditionModel(W.random_state_dict(W.unet_shapes(ucfg)), ucfg)
    with pytest.raises(lib.EdgeStyleHipError):
        unet(torch.zeros(1, 4, 16, 16), 1, torch.zeros(1, 77, ucfg.cross_attention_dim))


def test_pack_weight_layout():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(24, 16, 3, 3, generator=g)
    b = torch.randn(24, generator=g)
    pw = ops.pack_weight(w, b, torch.float32, "cpu")
    assert pw.w.shape == (128, 192) and pw.bn == 128 and pw.cout == 24 and pw.cin == 16 and pw.ksize == 3
    # K index = (ky*3+kx)*Cin + c
    assert float(pw.w[5, (1 * 3 + 2) * 16 + 7]) == float(w[5, 7, 1, 2])
    assert float(pw.w[24:].abs().max()) == 0 and float(pw.w[:, 144:].abs().max()) == 0 and torch.equal(pw.bias[:24], b)
    assert ops.choose_bn(320) == 160 and ops.choose_bn(640) == 128 and ops.choose_bn(960) == 160 and ops.choose_bn(4) == 128
    # Cin 4 -> 8 zero padding (conv_in), Cout 4 -> 8 zero rows (post_quant)
    p2 = ops.pack_weight(torch.ones(4, 4, 1, 1), torch.ones(4), torch.float32, "cpu", cin_pad=8, cout_pad=8)
    assert p2.cin == 8 and p2.cout == 8 and float(p2.w[:4, :4].sum()) == 16 and float(p2.w.sum()) == 16
    # GEGLU: packed rows in blocks of 32 = [16 hidden | 16 gate]
    inner = 64
    wg = torch.arange(2 * inner, dtype=torch.float32)[:, None].repeat(1, 8)
    pg = ops.pack_weight(wg, torch.arange(2 * inner, dtype=torch.float32), torch.float32, "cpu", geglu=True)
    rows = pg.w[: 2 * inner, 0].tolist()
    assert rows[:16] == list(range(0, 16)) and rows[16:32] == list(range(inner, inner + 16))
    assert rows[32:48] == list(range(16, 32)) and rows[48:64] == list(range(inner + 16, inner + 32))
    assert pg.bias[:32].tolist() == rows[:32]


def test_splitk_heuristic_bounds():
    for M, rows, bn, kpad in [(128, 1280, 128, 11520), (8192, 320, 160, 2880), (65536, 1280, 128, 11520), (2, 1280, 128, 320)]:
        s = ops.choose_splitk(M, rows, bn, kpad)
        assert 1 <= s <= kpad // 64


def test_plan_gemm_returns_legal_launches():
    """Every (M, Cout, K) of the SD1.5 path gets a launch the C ABI accepts: bn divides rows_padded, split-K only where
    it is allowed, 4-stage rings only with at most one workgroup per CU, the 64x64 tile only for small launches."""
    from tests import numerics as nm
    for M in (2, 128, 512, 896, 2048, 3584, 8192, 14336, 57344, 458752):
        for rows in (320, 640, 960, 1280, 1920, 2560, 3840):
            for kpad in (320, 640, 1280, 2880, 5760, 11520, 23040):
                for bns in ((160, 128, 64), (320, 160, 128), (128,)):
                    if not any(rows % b == 0 for b in bns):
                        continue
                    bn, sk, st = ops.plan_gemm(M, rows, kpad, bns=bns)
                    assert rows % bn == 0 and bn in bns
                    assert 1 <= sk <= max(1, kpad // 64) and st in (2, 4)
                    if bn == 64:
                        assert M <= nm.PLAN_SMALL_MAX_M or len(bns) == 1
                    if bn == 320:
                        assert st == 2 and M >= nm.PLAN_BIG_MIN_M
                    assert ops.plan_gemm(M, rows, kpad, bns=bns, allow_split=False)[1] == 1


def test_every_knob_bends_the_launch_choice_as_before():
    """es_launch_choose under the default knobs and with ONE knob changed.  The expected choices are literals: read off the descriptors that
    ops.conv_gemm recorded on the dry recorder, with that knob's module attribute set, at the commit before the policy moved into the library."""
    L, XS, F16, BF16 = lib.load(), "es_linear_xs", lib.ES_F16, lib.ES_BF16

    def choose(cin, cout, k, M, hw, facts, knobs, geglu=False):
        bn = 128 if geglu else ops.choose_bn(cout)
        pw = ops.PackedWeight(torch.empty(-(-cout // bn) * bn, k * k * cin, device="meta"), None, cout, cin, k, bn, geglu,
                              ln_colsum=torch.empty(0) if geglu else None)
        ch = lib.LaunchChoice()
        q = ops.launch_query(M, hw, pw, C1=cin, src_numel=M * cin, **facts)
        if L.es_launch_choose(ctypes.byref(q), ctypes.byref(ops.launch_knobs(**knobs)), ctypes.byref(ch)) != 0:
            return L.es_last_error()
        return XS if ch.route == lib.ROUTE_LINEAR_XS else (ch.bn, ch.splitk, ch.stages, ch.waves, ch.xcd_m_fastest, ch.gn_partials, ch.wide)
    res, gn = dict(has_residual=1), dict(gn_groups=32)
    table = [   # (cin, cout, ksize, M, hw, call facts): {changed knob: choice}
        ((320, 960, 1, 16384, 16384, {}), {(): XS, ("xs_enabled", 0): (160, 1, 2, 8, 0, 0, 0)}),
        ((320, 960, 1, 1024, 1024, {}), {(): (64, 1, 2, 0, 0, 0, 0), ("xs_min_m", 0): XS}),
        ((320, 320, 1, 32768, 4096, res), {(): XS, ("xs_residual", 0): (160, 1, 2, 8, 0, 0, 0)}),
        ((320, 320, 1, 256, 256, {}), {(): (64, 1, 2, 0, 1, 0, 0), ("small_tile", 0): (160, 1, 2, 8, 1, 0, 0), ("force_waves", 8): (160, 1, 2, 8, 1, 0, 0)}),
        ((1280, 1280, 1, 4096, 4096, {}), {(): (128, 1, 2, 8, 0, 0, 0), ("eight_waves", 0): (128, 1, 2, 0, 0, 0, 0), ("xcd_order", 1): (128, 1, 2, 8, 1, 0, 0)}),
        ((320, 320, 3, 57344, 4096, {}), {(): (320, 1, 2, 0, 0, 0, 0), ("big_tile", 0): (160, 1, 2, 0, 0, 0, 0)}),
        ((320, 640, 3, 57344, 4096, {}), {(): (320, 1, 2, 0, 0, 0, 0), ("force_bn", 128): (128, 1, 2, 0, 0, 0, 0)}),
        ((1280, 1280, 1, 1024, 1024, {}), {(): (64, 1, 4, 0, 1, 0, 0), ("deep_ring", 0): (64, 1, 2, 0, 1, 0, 0)}),
        ((320, 320, 3, 8192, 4096, gn), {(): (160, 3, 2, 0, 0, 0, 0), ("gn_handover", 1): (160, 3, 2, 0, 0, 1, 0), ("gn_handover", 2): (160, 3, 2, 0, 0, 1, 0)}),
        ((1280, 1280, 3, 512, 256, gn), {(): (128, 12, 2, 0, 0, 0, 0), ("gn_handover", 1): (128, 12, 2, 0, 0, 0, 0), ("gn_handover", 2): (128, 12, 2, 0, 0, 1, 0)}),
        ((320, 320, 1, 32768, 4096, dict(res, wide=1, dtype=F16)), {(): XS, ("wide_stream", 1): (160, 1, 2, 8, 0, 0, 1)}),
        ((320, 320, 1, 32768, 4096, dict(res, wide=1, dtype=BF16)), {(): (160, 1, 2, 8, 0, 0, 1), ("wide_stream", 0): XS}),
    ]
    for call, want in table:
        for knob, choice in want.items():
            assert choose(*call, dict([knob] if knob else [])) == choice, (call, knob)
    # the 28672 x 1280 -> 10240 GEGLU of the 64 x 64 level (LayerNorm folded in)
    assert choose(1280, 10240, 1, 28672, 4096, {}, {}, geglu=True) == (256, 1, 2, 0, 0, 0, 0)
    assert choose(1280, 10240, 1, 28672, 4096, {}, dict(big_tile_256=0), geglu=True) == (128, 1, 2, 8, 0, 0, 0)
    assert b"fits no N tile" in choose(320, 320, 3, 57344, 4096, {}, dict(force_bn=128))          # (rows_padded 320)


_KNOB_DEFAULTS = dict(xs_enabled=1, xs_residual=1, xs_min_m=8192, big_tile=1, big_tile_256=1, small_tile=1, eight_waves=1, deep_ring=1,
                      gn_handover=0, wide_stream=-1, gn_fold=1, force_bn=0, force_waves=0, force_stages=0, xcd_order=-1)


def test_default_knobs_are_the_python_hosts_in_a_process_without_switches():
    """es_launch_default_knobs: the values include/edgestyle_hip.h states, and - in a fresh child whose environment holds no ES_* variable,
    which imports the package and loads the library and nothing else - ops.launch_knobs() field by field."""
    import json
    import subprocess
    import sys
    k = lib.LaunchKnobs(*([77] * len(lib.LaunchKnobs._fields_)))
    lib.load().es_launch_default_knobs(ctypes.byref(k))
    assert {n: getattr(k, n) for n, _ in lib.LaunchKnobs._fields_} == _KNOB_DEFAULTS
    lib.load().es_launch_default_knobs(None)                      # (a null pointer is ignored)
    code = ("import ctypes, json\nfrom edgestyle_amd import lib, ops\nk = lib.LaunchKnobs()\nlib.load().es_launch_default_knobs(ctypes.byref(k))\n"
            "f = [n for n, _ in lib.LaunchKnobs._fields_]\nh = ops.launch_knobs()\n"
            "print(json.dumps([{n: getattr(k, n) for n in f}, {n: getattr(h, n) for n in f}]))")
    env = {n: v for n, v in os.environ.items() if not n.startswith("ES_")}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    native, host = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(native) == set(_KNOB_DEFAULTS)
    for name in native:
        assert native[name] == host[name] == _KNOB_DEFAULTS[name], (name, native[name], host[name])


def test_encoder_towers_choose_the_same_launches_under_the_shared_defaults():
    """The CLIP towers (csrc/encoder.h) used to fill their knobs by hand - the tiles, eight waves and the deep ring on, the rest 0 - and now
    start from es_launch_default_knobs with es_linear_xs off, which also leaves xs_residual, gn_fold and xs_min_m set and wide_stream at
    auto.  None of those is read without xs_enabled or a `wide` call: over the towers' layer shapes, queried as encoder.h's choose() does,
    the two knob sets give the same return code and the same es_launch_choice, byte for byte."""
    L = lib.load()
    old = lib.LaunchKnobs(big_tile=1, big_tile_256=1, small_tile=1, eight_waves=1, deep_ring=1, xcd_order=-1)
    new = lib.LaunchKnobs()
    L.es_launch_default_knobs(ctypes.byref(new))
    new.xs_enabled = 0
    assert bytes(old) != bytes(new)
    n = 0
    for hidden in (128, 768, 1024):
        inter = 4 * hidden
        for cout, cin in ((3 * hidden, hidden), (hidden, hidden), (inter, hidden), (hidden, inter)):      # q|k|v, out_proj, fc1, fc2
            bn = ops.choose_bn(cout)
            rows_padded, kpad = -(-cout // bn) * bn, -(-cin // 64) * 64
            for M in (77, 2 * 77, 16 * 77, 50, 257, 2 * 257, 16 * 257):
                for ln in (0, 1):
                    for res in (0, 1):
                        for act in (lib.ACT_NONE, lib.ACT_SILU):
                            for dtype in (lib.ES_F16, lib.ES_BF16):
                                q = lib.LaunchQuery(M=M, hw=1, w_numel=rows_padded * kpad, src_numel=M * cin, ksize=1, stride=1, C1=cin,
                                                    rows_padded=rows_padded, kpad=kpad, cin=cin, cout=cout, has_ln=ln, act=act, has_residual=res,
                                                    residual_dense=1, unit_scale=1, x_rep=1, dtype=dtype)
                                got = []
                                for knobs in (old, new):
                                    k = lib.LaunchKnobs.from_buffer_copy(knobs)
                                    if act != lib.ACT_NONE:
                                        k.big_tile_256 = 0
                                    ch = lib.LaunchChoice(*([-1] * 8))
                                    got.append((L.es_launch_choose(ctypes.byref(q), ctypes.byref(k), ctypes.byref(ch)), bytes(ch)))
                                assert got[0] == got[1] and got[0][0] == 0, (hidden, cout, cin, M, ln, res, act, dtype, got)
                                n += 1
    assert n == 3 * 4 * 7 * 16


def test_linear_xs_slice_rule_of_the_library_equals_its_mirror():
    """es_launch_xs_slices (what ops.linear_xs and es_load_weights both ask) against tests/numerics.py xs_slices_reference, the arithmetic the
    two hosts used to write out: every row count around a 256-row block and up to 2^20, both K, Cout from one line (the kernel runs fewer
    than the four lines the policy routes to it, and its tests launch them) to 5120, GEGLU on and off, the slice count forced and not;
    every answer is a cut es_linear_xs accepts; what that kernel does not run is refused with a text."""
    from tests import numerics as nm
    L = lib.load()
    ns, cps = ctypes.c_int32(), ctypes.c_int32()
    n = 0
    for M in (1, 255, 256, 257, 4096, 8192, 57344, 458752, 1 << 20):
        for K in (320, 640):
            for geglu in (False, True):
                ch = 64 if K == 320 else 32
                pline = 128 // (ch if geglu else 2 * ch)
                line = ch * pline
                for cout in sorted({line * i for i in (1, 2, 3, 4, 5, 7, 8, 15, 16, 30)} | {c for c in (320, 640, 960, 1280, 1920, 2560, 5120) if c % line == 0}):
                    for force in (0, 1, 3, 1000):
                        want = nm.xs_slices_reference(M, K, cout, geglu, force)
                        assert L.es_launch_xs_slices(M, K, cout, int(geglu), force, ctypes.byref(ns), ctypes.byref(cps)) == 0, (M, K, cout, geglu, force)
                        assert (ns.value, cps.value) == want, (M, K, cout, geglu, force, ns.value, cps.value, want)
                        total = cout // ch                   # (es_linear_xs: slices cover Cout in whole output lines, none empty)
                        assert cps.value % pline == 0 and ns.value * cps.value >= total > (ns.value - 1) * cps.value
                        if force:
                            assert ns.value <= force
                        n += 1
    assert n > 1500
    for M, K, cout, geglu in ((0, 320, 960, 0), (4096, 1280, 1280, 0), (4096, 320, 96, 0), (4096, 640, 32, 0), (4096, 320, 0, 0), (4096, 640, 2560 + 32, 1)):
        assert nm.xs_slices_reference(M, K, cout, bool(geglu)) is None
        assert L.es_launch_xs_slices(M, K, cout, geglu, 0, ctypes.byref(ns), ctypes.byref(cps)) == -1 and b"es_launch_xs_slices: " in L.es_last_error()
    assert L.es_launch_xs_slices(4096, 320, 960, 0, 0, None, ctypes.byref(cps)) == -1 and b"null argument" in L.es_last_error()


def test_layer_norm_fold_algebra():
    """pack_weight_ln: Linear(LayerNorm(x)) == rstd (x (W gamma)^T - mean colsum) + (W beta + b), with the column sums
    taken from the rounded packed weights (what the kernel's epilogue computes)."""
    g = torch.Generator().manual_seed(5)
    M, C, Cout = 37, 128, 192
    x = torch.randn(M, C, generator=g) * 2 + 1
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    w, b = torch.randn(Cout, C, generator=g) / 11, torch.randn(Cout, generator=g) * 0.1
    pw = ops.pack_weight_ln(w, b, gamma, beta, 1e-5, torch.float32, "cpu")
    assert pw.ln_colsum is not None and pw.ln_colsum.shape[0] == pw.rows_padded
    mean = x.mean(1, keepdim=True)
    rstd = (x.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    y = rstd * (x @ pw.w[:Cout, :C].T - mean * pw.ln_colsum[None, :Cout]) + pw.bias[None, :Cout]
    ref = torch.nn.functional.linear(torch.nn.functional.layer_norm(x, (C,), gamma, beta, 1e-5), w, b)
    assert float((y - ref).abs().max()) < 1e-4


def test_tail_and_ffo_fold_algebra():
    """The two weight folds of this path restated on the CPU from the packed tensors themselves.
    (a) ops.pack_weight_tail: conv3x3(h) + conv1x1(t) == one GEMM over K = (ky,kx,c) taps of h followed by t's channels at
        the output pixel (ResnetBlock2D conv2 + conv_shortcut);
    (b) engine.Transformer.ffo: proj_out(ff2(f) + tok) + x == [Wp Wf | Wp] [f | tok] + (Wp bf + bp) + x."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(9)
    N, C, Ct, Cout, H = 2, 64, 128, 96, 5
    h, t = torch.randn(N, C, H, H, generator=g), torch.randn(N, Ct, H, H, generator=g)
    w3, w1 = torch.randn(Cout, C, 3, 3, generator=g) / 24, torch.randn(Cout, Ct, 1, 1, generator=g) / 11
    b = torch.randn(Cout, generator=g)
    pw = ops.pack_weight_tail(w3, w1, b, torch.float32, "cpu")
    assert pw.ctail == Ct and pw.cin == C and pw.ksize == 3 and pw.kpad == 9 * C + Ct
    cols = F.unfold(h, 3, padding=1)                                  # [N, C*9, HW], index c*9 + tap
    cols = cols.view(N, C, 9, H * H).permute(0, 3, 2, 1).reshape(N, H * H, 9 * C)      # tap-major (ky,kx,c), like the kernel's K
    a = torch.cat([cols, t.permute(0, 2, 3, 1).reshape(N, H * H, Ct)], 2)
    y = (a @ pw.w[:Cout].T + pw.bias[:Cout]).permute(0, 2, 1).reshape(N, Cout, H, H)
    ref = F.conv2d(h, w3, None, padding=1) + F.conv2d(t, w1, None) + b[None, :, None, None]
    assert float((y - ref).abs().max()) < 1e-4
    with pytest.raises(Exception):
        ops.pack_weight_tail(w3[:, :40], w1, b, torch.float32, "cpu")      # 40 input channels: not a multiple of 64

    Cm, M = 64, 11
    f, tok, x = torch.randn(M, 4 * Cm, generator=g), torch.randn(M, Cm, generator=g), torch.randn(M, Cm, generator=g)
    wf, bf = torch.randn(Cm, 4 * Cm, generator=g) / 16, torch.randn(Cm, generator=g) * 0.1
    wp, bp = torch.randn(Cm, Cm, generator=g) / 8, torch.randn(Cm, generator=g) * 0.1
    ref = F.linear(F.linear(f, wf, bf) + tok, wp, bp) + x
    wc = torch.cat([wp.double() @ wf.double(), wp.double()], 1).float()
    bc = (wp.double() @ bf.double() + bp.double()).float()
    pwc = ops.pack_weight(wc, bc, torch.float32, "cpu")
    y = torch.cat([f, tok], 1) @ pwc.w[:Cm, : 5 * Cm].T + pwc.bias[:Cm] + x
    assert float((y - ref).abs().max()) < 1e-4


def test_controllora_state_dict_is_lora_plus_zero_convs_only():
    ucfg = C.tiny_unet()
    ws = make_weights(ucfg, C.tiny_vae())
    unet = UNet2DConditionModel(ws["unet"], ucfg)
    net = ControlLoRAModel(ws["lora0"], ucfg, lora_linear_rank=4, uses_vae=True)
    with pytest.raises(lib.EdgeStyleHipError):
        net.full_state_dict()                                   # tie_weights first (TT:259-261)
    net.tie_weights(unet)
    full = net.full_state_dict()
    assert full["down_blocks.1.resnets.0.conv1.weight"] is ws["unet"]["down_blocks.1.resnets.0.conv1.weight"]
    saved = net.state_dict()
    assert set(saved) == set(W.controllora_saved_shapes(ucfg, 4))          # CL:600-606
    assert all(k.split(".")[0] not in W.SKIP_LAYERS or ".lora_layer." in k for k in saved)
    fused = net.fuse()
    assert isinstance(fused, FusedControlLoRAModel) and not any(".lora_layer." in k for k in fused.state_dict())
    k = "mid_block.attentions.0.transformer_blocks.0.ff.net.2"
    want = ws["unet"][k + ".weight"] + ws["lora0"][k + ".lora_layer.up.weight"] @ ws["lora0"][k + ".lora_layer.down.weight"]
    assert torch.allclose(fused.state_dict()[k + ".weight"], want, atol=1e-6)
    assert torch.equal(ws["unet"][k + ".weight"], unet.state_dict()[k + ".weight"])   # tied UNet tensor untouched


def test_multicontrolnet_directory_layout_round_trip(tmp_path):
    """save_pretrained / from_pretrained (MC:213-282, MC:289-430) incl. load_pattern de-duplication and errors"""
    ucfg, vcfg = C.tiny_unet(), C.tiny_vae()
    ws = make_weights(ucfg, vcfg)
    unet = UNet2DConditionModel(ws["unet"], ucfg)
    vae = AutoencoderKL(ws["vae"], vcfg)
    pose = ControlNetModel(ws["openpose"], ucfg)
    l0 = ControlLoRAModel(ws["lora0"], ucfg, lora_linear_rank=4, uses_vae=True)
    l1 = ControlLoRAModel(ws["lora1"], ucfg, lora_linear_rank=4, uses_vae=True)
    mc = EdgeStyleMultiControlNetModel([l0, pose, l1, pose, l1, pose])
    mc.load_state_dict(ws["fusion"])
    d = str(tmp_path / "controlnet")
    mc.save_pretrained(d, save_pattern=C.CONTROLNET_PATTERN)
    assert sorted(os.listdir(d)) == ["controlnet_0", "controlnet_1", "diffusion_pytorch_model.safetensors"]
    with pytest.raises(ValueError):
        EdgeStyleMultiControlNetModel.from_pretrained(d, controlnet_class=ControlLoRAModel)              # no load_pattern
    with pytest.raises(ValueError):
        EdgeStyleMultiControlNetModel.from_pretrained(d, controlnet_class=ControlLoRAModel,
                                                      load_pattern=C.CONTROLNET_PATTERN,
                                                      static_controlnets=[None, pose, None, pose, None, pose])  # no vae
    with pytest.raises(ValueError):
        EdgeStyleMultiControlNetModel.from_pretrained(d, controlnet_class=ControlLoRAModel, vae=vae,
                                                      load_pattern=C.CONTROLNET_PATTERN)                 # nets missing
    with pytest.raises(ValueError):
        EdgeStyleMultiControlNetModel.from_pretrained(str(tmp_path / "nope"), load_pattern=[0])
    m2 = EdgeStyleMultiControlNetModel.from_pretrained(d, vae=vae, controlnet_class=ControlLoRAModel,
                                                       load_pattern=C.CONTROLNET_PATTERN,
                                                       static_controlnets=[None, pose, None, pose, None, pose])
    assert m2.nets[2] is m2.nets[4] and m2.nets[1] is pose and m2.nets[0] is not m2.nets[2]    # MC:379-398
    assert [len(p) for _, p in m2.groups()] == [1, 3, 2]
    for k, v in ws["fusion"].items():
        assert torch.equal(m2.state_dict()[k], v)
    for k, v in ws["lora1"].items():
        assert torch.equal(m2.nets[2].state_dict()[k], v)
    assert m2.nets[0].config.uses_vae and m2.nets[0].config.lora_linear_rank == 4
    bad = dict(ws["fusion"])
    bad.pop("multi_controlnet_mid_block.third_conv.bias")
    with pytest.raises(RuntimeError):
        m2.load_state_dict(bad)
    # unet / vae round trip + config mapping from a diffusers-style config.json
    unet.save_pretrained(str(tmp_path / "sd" / "unet"))
    u2 = UNet2DConditionModel.from_pretrained(str(tmp_path / "sd"), subfolder="unet", torch_dtype=torch.float16)
    assert u2.cfg == ucfg and torch.equal(u2.state_dict()["conv_in.weight"], ws["unet"]["conv_in.weight"])
    cfg = unet_config_from_json({"block_out_channels": [320, 640, 1280, 1280], "attention_head_dim": 8,
                                 "cross_attention_dim": 768, "down_block_types": ["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"]})
    assert cfg == C.sd15_unet()


def test_ddim_scheduler_tables_match_oracle():
    from oracle import sd15_oracle as O
    s, o = DDIMScheduler(), O.DDIM()
    assert s.set_timesteps(50).tolist() == o.set_timesteps(50).tolist()
    tab = s.coef_table()
    assert tab.shape == (50, 4)
    x, e = torch.randn(1, 4, 8, 8), torch.randn(1, 4, 8, 8)
    for i in (0, 17, 49):
        c = tab[i]
        mine = c[2] * (x - c[1] * e) / c[0] + c[3] * e
        assert torch.allclose(mine, o.step(e, int(s.timesteps[i]), x), atol=1e-5)
    with pytest.raises(ValueError):
        s.set_timesteps(2000)


def test_shard_ranges_cover_and_seeds_are_world_size_independent():
    for n, w in [(64, 8), (64, 1), (10, 4), (3, 8), (0, 2)]:
        spans = [shard_range(n, r, w) for r in range(w)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1
    assert [shard_seed(42, r, 8) for r in range(8)] == [42 + 8 * r for r in range(8)]
    with pytest.raises(ValueError):
        shard_range(4, 4, 4)


def test_unipc_coefficient_table_reproduces_oracle_trajectory():
    """The product scheduler only exports linear-recombination coefficients (the arithmetic is es_cfg_unipc_step);
    applying them in float64 must reproduce the oracle's UniPC restatement step for step."""
    from oracle import sd15_oracle as O
    from edgestyle_amd.schedulers import UniPCMultistepScheduler
    for n in (50, 5, 2):
        s = UniPCMultistepScheduler.from_config({"steps_offset": 1, "timestep_spacing": "leading", "foo": 1})
        ts = s.set_timesteps(n)
        o = O.UniPC()
        assert o.set_timesteps(n).tolist() == ts.tolist()
        tab = s.coef_table().double()
        assert tab.shape == (n, 12) and float(tab[0, 2]) == 0.0 and float(tab[1, 2]) == 1.0
        g = torch.Generator().manual_seed(n)
        xo = torch.randn(1, 4, 8, 8, generator=g)
        xm, last, m0, m1 = xo.double(), torch.zeros(1, 4, 8, 8).double(), torch.zeros(1, 4, 8, 8).double(), torch.zeros(1, 4, 8, 8).double()
        for i, t in enumerate(ts.tolist()):
            eps = torch.randn(1, 4, 8, 8, generator=g)
            xo = o.step(eps, t, xo)
            c = tab[i]
            x0 = (xm - c[1] * eps.double()) / c[0]
            xc = c[3] * last + c[4] * m0 + c[5] * m1 + c[6] * x0 if c[2] != 0 else xm
            xm, m1, m0, last = c[7] * xc + c[8] * x0 + c[9] * m0, m0, x0, xc
            assert float((xm.float() - xo).abs().max() / xo.abs().max()) < 1e-5
    # exactness property of the solver itself: with the true noise as model output it stays on the marginal
    o = O.UniPC()
    ts = o.set_timesteps(20)
    x0t, nz = torch.randn(1, 4, 8, 8), torch.randn(1, 4, 8, 8)
    a, sg = o._alpha_sigma(o.sigmas[0])
    x = (a * x0t + sg * nz).float()
    for t in ts.tolist():
        x = o.step(nz, t, x)
    a, sg = o._alpha_sigma(o.sigmas[-1])
    assert float((x - (a * x0t + sg * nz).float()).abs().max()) < 1e-4


# ---------------------------------------------------------------------------------------------------------------
# serving loop (edgestyle_amd/serve.py): host logic with a stand-in pipeline
class _FakePipe:
    """Per-sample deterministic 'pipeline': image_i depends only on request i's own inputs."""

    def __init__(self, fail_on_steps=None, delay=0.0):
        self.calls = []
        self.fail_on_steps, self.delay = fail_on_steps, delay

    def __call__(self, prompt_embeds, negative_prompt_embeds, image, latents, guidance_scale, num_inference_steps,
                 control_guidance_start, control_guidance_end, output_type):
        import time
        import types
        assert output_type == "pt" and len(image) == 6
        B = latents.shape[0]
        assert all(t.shape[0] == B for t in (prompt_embeds, negative_prompt_embeds, *image))
        self.calls.append((B, num_inference_steps, guidance_scale))
        if self.fail_on_steps == num_inference_steps:
            raise RuntimeError("boom")
        time.sleep(self.delay)
        per = latents.mean(dim=(1, 2, 3)) + prompt_embeds.mean(dim=(1, 2)) - negative_prompt_embeds.mean(dim=(1, 2)) \
            + sum(im.mean(dim=(1, 2, 3)) * (k + 1) for k, im in enumerate(image)) + guidance_scale
        return types.SimpleNamespace(images=per[:, None, None, None].expand(B, 3, 8, 8).clone())


def _request(seed, steps=50, gs=7.5, hw=16):
    from edgestyle_amd.serve import TryOnRequest
    g = torch.Generator().manual_seed(1000 + seed)
    return TryOnRequest([torch.randn(1, 3, hw, hw, generator=g) for _ in range(6)], torch.randn(1, 77, 32, generator=g),
                        torch.randn(1, 77, 32, generator=g), gs, steps, seed)


def test_service_batches_compatible_requests_and_results_do_not_depend_on_the_batch():
    from edgestyle_amd.serve import TryOnService
    solo_pipe = _FakePipe()
    solo = TryOnService(solo_pipe, max_batch=1, max_wait_s=0.0)
    want = [solo.submit(_request(s)).result(timeout=10) for s in range(5)]
    solo.shutdown()
    assert [c[0] for c in solo_pipe.calls] == [1] * 5

    pipe = _FakePipe(delay=0.05)
    svc = TryOnService(pipe, max_batch=8, max_wait_s=0.3, batch_sizes=(1, 2, 4, 8))
    futs = [svc.submit(_request(s)) for s in range(5)]
    got = [f.result(timeout=10) for f in futs]
    svc.shutdown()
    for a, b in zip(got, want):
        assert a.shape == (1, 3, 8, 8) and torch.allclose(a, b, atol=1e-6)
    # five compatible requests: captured batch sizes only -> 4 + 1, oldest first
    assert sorted(c[0] for c in pipe.calls) == [1, 4] and pipe.calls[0][0] == 4
    assert svc.stats["images"] == 5 and svc.stats["calls"] == 2


def test_service_keeps_incompatible_requests_apart_and_survives_a_failing_batch():
    from edgestyle_amd.serve import TryOnService
    pipe = _FakePipe(fail_on_steps=7)
    svc = TryOnService(pipe, max_batch=4, max_wait_s=0.2)
    a = [svc.submit(_request(s, steps=50)) for s in range(2)]
    b = [svc.submit(_request(s, steps=7)) for s in range(2)]          # this batch raises inside the pipeline
    c = [svc.submit(_request(9, steps=50, gs=3.0))]
    for f in a + c:
        assert f.result(timeout=10).shape == (1, 3, 8, 8)
    for f in b:
        with pytest.raises(RuntimeError, match="boom"):
            f.result(timeout=10)
    svc.shutdown()
    assert (2, 50, 7.5) in pipe.calls and (2, 7, 7.5) in pipe.calls and (1, 50, 3.0) in pipe.calls
    with pytest.raises(RuntimeError):
        svc.submit(_request(1))
    with pytest.raises(ValueError):
        TryOnService(pipe, batch_sizes=(2, 4))


def test_service_latents_depend_on_the_request_seed_only():
    from edgestyle_amd.serve import latents_for
    a, b = latents_for(42, 4, 8, 8), latents_for(42, 4, 8, 8)
    assert torch.equal(a, b) and not torch.equal(a, latents_for(43, 4, 8, 8)) and a.shape == (1, 4, 8, 8)


def test_best_embeddings_prompt_picker():
    """BestEmbeddings (model/utils.py:647-684): top-2 colours + top-2 items by CLIP image-text probability, joined into
    "edgestyle, c1, c2, i1, i2"; here with a stand-in model whose logits are known."""
    from types import SimpleNamespace
    from edgestyle_amd.prompts import BestEmbeddings, DEFAULT_COLORS

    class Proc:
        def __call__(self, text, images, return_tensors, padding):
            return {"text": text, "n_images": len(images)}

    class Model:
        device = None

        def __call__(self, text, n_images):
            # image i prefers entries i, i+1, ... (descending logits from index i, cyclic)
            n = len(text)
            logits = torch.stack([torch.roll(torch.arange(n, 0, -1).float(), i) for i in range(n_images)])
            return SimpleNamespace(logits_per_image=logits)

    colors = ["red", "green", "blue", "black"]
    items = ["dress", "shirt", "coat"]
    be = BestEmbeddings(Model(), Proc(), colors=colors, clothing_items=items)
    assert be([object(), object()]) == ["edgestyle, red, green, dress, shirt", "edgestyle, green, blue, shirt, coat"]
    assert BestEmbeddings(Model(), Proc()).colors == DEFAULT_COLORS
    assert be.find_best(colors, [object()], n=3) == [["red", "green", "blue"]]


def test_pointer_field_tables_match_the_descriptor_structs():
    """es_plan_pointer_fields (what es_ctx_save_ranges relocates by, instead of guessing pointers from bit patterns): for every
    descriptor struct mirrored in edgestyle_amd/lib.py, the library's table names exactly the pointer-typed fields of the
    struct - no more, no fewer -, each 8-byte aligned and inside the record, each with a use (1 reads, 2 writes, 3 both)."""
    L = lib.load()

    def table(kind):
        offs, uses = (ctypes.c_int32 * 64)(), (ctypes.c_int32 * 64)()
        elem = ctypes.c_int32(-1)
        n = L.es_plan_pointer_fields(kind, offs, uses, 64, ctypes.byref(elem))
        assert 0 <= n <= 64
        return [(offs[i], uses[i]) for i in range(n)], elem.value

    def struct_ptr_offsets(st):
        out = set()
        for name, tp in st._fields_:
            f = getattr(st, name)
            if tp is ctypes.c_void_p or (isinstance(tp, type) and issubclass(tp, ctypes._Pointer)):
                out.add(f.offset)
            elif isinstance(tp, type) and issubclass(tp, ctypes.Array) and (tp._type_ is ctypes.c_void_p):
                out.update(f.offset + 8 * i for i in range(tp._length_))
        return out

    # op kinds of csrc/plan.h: 1 conv_gemm, 2 linear_xs, 3 attention, 4 group_norm, 6 layer_norm_grouped, 7 / 8 fusion block(s)
    for kind, st in ((1, lib.GemmDesc), (2, lib.XsDesc), (3, lib.AttnDesc), (4, lib.GnDesc), (6, lib.LnDesc), (7, lib.FusionDesc),
                     (8, lib.FusionDesc)):
        fl, elem = table(kind)
        assert elem == (ctypes.sizeof(st) if kind == 8 else 0)
        assert {o for o, _ in fl} == struct_ptr_offsets(st), (kind, sorted(o for o, _ in fl), sorted(struct_ptr_offsets(st)))
        assert len({o for o, _ in fl}) == len(fl) and all(o % 8 == 0 and o + 8 <= ctypes.sizeof(st) and u in (1, 2, 3) for o, u in fl)
    # the outputs are marked as written
    g = dict(table(1)[0])
    assert g[lib.GemmDesc.out.offset] == 2 and g[lib.GemmDesc.w.offset] == 1 and g[lib.GemmDesc.workspace.offset] == 3
    # small argument records (memcpy, incr, ...) and markers / unknown kinds
    assert len(table(18)[0]) == 2 and len(table(16)[0]) == 1 and table(64) == ([], 0) and table(999) == ([], 0)


def test_graph_hazard_guard_sees_a_queue_intercepting_profiler():
    """es_ctx_graph_hazard (csrc/plan.hip): under rocprofv3 (ROCP_TOOL_LIBRARIES / a rocprofiler library in LD_PRELOAD) without
    DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 the HIP runtime faults below hipGraphLaunch (profiles/r04_rocprof_graph_fault.txt); the
    context then replays its plans launch by launch.  One process per environment: the answer is latched at first use."""
    import subprocess
    import sys
    code = ("import ctypes, sys; sys.path.insert(0, %r); from edgestyle_amd import lib; "
            "print(ctypes.CDLL(lib.LIB_PATH).es_ctx_graph_hazard())" % ROOT)

    def ask(**env):
        e = {k: v for k, v in os.environ.items() if k not in ("ROCP_TOOL_LIBRARIES", "LD_PRELOAD", "DEBUG_CLR_GRAPH_PACKET_CAPTURE")}
        e.update(env)
        r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-500:]
        return int(r.stdout.strip().splitlines()[-1]), r.stderr
    assert ask()[0] == 0
    v, err = ask(ROCP_TOOL_LIBRARIES="/opt/rocm/lib/rocprofiler-sdk/librocprofiler-sdk-tool.so")
    assert v == 1 and "launch by launch" in err
    assert ask(ROCP_TOOL_LIBRARIES="/opt/rocm/lib/rocprofiler-sdk/librocprofiler-sdk-tool.so", DEBUG_CLR_GRAPH_PACKET_CAPTURE="0")[0] == 0


def test_big_tile_epilogue_forms():
    """es_conv_gemm8p_form_ok: the epilogue forms the 256 x 320 tile implements for splitk == 1 (both hosts ask before they fix
    bn = 320, so the planned / recorded / reported tile is the tile that runs)."""
    L = lib.load()
    ok = L.es_conv_gemm8p_form_ok
    assert ok(lib.ACT_NONE, 320, 0, 4096, 0) == 1 and ok(lib.ACT_NONE, 320, 0, 4096, 1) == 1
    assert ok(lib.ACT_NONE, 320, 1, 4096, 0) == 1          # one time-embedding row per 128-pixel half
    assert ok(lib.ACT_NONE, 320, 1, 4096, 1) == 0          # ... not beside a residual
    assert ok(lib.ACT_NONE, 320, 1, 64, 0) == 0            # ... nor when a half spans samples
    assert ok(lib.ACT_SILU, 320, 0, 4096, 0) == 0 and ok(lib.ACT_NONE, 4, 0, 4096, 0) == 0


class _DryPlan:
    """A recording plan in dry mode (es_plan_set_dry(1)): every C-ABI compute call validates its descriptor and records it, and
    launches nothing - the entry points' checks can be exercised with host buffers, without a GPU."""

    def __enter__(self):
        self.L = lib.load()
        self.plan = ctypes.c_void_p(self.L.es_plan_create())
        assert self.L.es_plan_begin_record(self.plan) == 0
        self.was = self.L.es_plan_set_dry(1)
        return self

    def __exit__(self, *a):
        self.L.es_plan_set_dry(self.was)
        self.L.es_plan_end_record(self.plan)
        self.L.es_plan_destroy(self.plan)

    def size(self):
        return self.L.es_plan_size(self.plan)


def test_linear_xs_refuses_a_weight_group_boundary_inside_a_group_norm_sample():
    """es_linear_xs with GroupNorm in front (gn_part) and several weight groups: a row block takes its statistics from one sample
    and its gamma / beta / weights from one group, so every group must end on a sample boundary ((mt_end * 128) % gn_hw == 0).
    Host-side validation, through the dry recorder with host buffers."""
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)

    def desc(mt_end, hw):
        d = lib.XsDesc()
        d.x = d.out = d.gn_part = p
        d.M, d.K, d.Cout, d.rows_padded, d.ldo = 8 * 1024, 320, 320, 320, 320
        d.nslices, d.chunks_per_slice, d.dtype = 1, 5, lib.ES_F16
        d.gn_groups, d.gn_nchunk, d.gn_hw, d.gn_eps = 32, 4, hw, 1e-6
        d.ngroups = len(mt_end)
        for g, e in enumerate(mt_end):
            d.mt_end[g] = e
            d.w_g[g] = d.bias_g[g] = d.gn_gamma_g[g] = d.gn_beta_g[g] = p
        return d

    with _DryPlan() as dry:
        L = dry.L
        # 8 samples of 1024 rows; groups of 2 + 6 samples: accepted, recorded, not launched
        assert L.es_linear_xs(ctypes.byref(desc([16, 64], 1024)), None) == 0 and dry.size() == 1
        # the first group ends after 1.5 samples (whole 256-row blocks, as the ungrouped check demands): refused, nothing recorded
        assert L.es_linear_xs(ctypes.byref(desc([12, 64], 1024)), None) == -1
        assert b"es_linear_xs: gn_part needs weight groups of whole samples" in L.es_last_error()
        # ... also when a later boundary is the misplaced one
        assert L.es_linear_xs(ctypes.byref(desc([16, 26, 64], 1024)), None) == -1
        assert b"whole samples" in L.es_last_error()
        # samples of 256 rows: every 256-row block boundary is a sample boundary
        assert L.es_linear_xs(ctypes.byref(desc([12, 26, 64], 256)), None) == 0
        assert dry.size() == 2


def test_conv_gemm_refuses_an_empty_problem_before_it_sizes_the_launch():
    """es_conv_gemm: N, Hout, Wout, Cout >= 1 are checked BEFORE the launch is sized for the 32-bit buffer offsets (oversize() and
    run_samples() divide by the sample size and by Hout * Wout * (rows_padded / 8)): a malformed descriptor returns -1 with
    a message.  The descriptors below are oversize ones (operand limit lowered) with split-K, the form that reached the divisions."""
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)

    def desc(**kw):
        d = lib.GemmDesc()
        d.x = d.w = d.out = d.workspace = p
        d.N, d.Hsrc, d.Wsrc, d.C1 = 4, 16, 16, 1280
        d.Hout, d.Wout, d.Cout, d.rows_padded, d.Kpad = 16, 16, 1280, 1280, 9 * 1280
        d.ksize, d.stride, d.pad, d.splitk, d.bn, d.dtype = 3, 1, 1, 2, 128, lib.ES_F16
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    with _DryPlan() as dry:
        L = dry.L
        prev = L.es_set_operand_limit(1 << 20)             # 655 KB per sample: the 4-sample launch is cut into single samples
        try:
            assert L.es_conv_gemm(ctypes.byref(desc()), None) == 0 and dry.size() == 1
            for bad in (dict(N=0), dict(Hout=0), dict(Wout=0), dict(Hout=0, Wout=0), dict(N=-1), dict(Cout=0, rows_padded=0)):
                assert L.es_conv_gemm(ctypes.byref(desc(**bad)), None) == -1, bad
                assert L.es_last_error() == b"es_conv_gemm: empty problem", (bad, L.es_last_error())
            # rows_padded is checked against the N tile before anything divides by it, too
            assert L.es_conv_gemm(ctypes.byref(desc(rows_padded=1284)), None) == -1
            assert L.es_last_error() == b"es_conv_gemm: bad rows_padded"
            assert dry.size() == 1                          # a rejected call never enters the plan
        finally:
            L.es_set_operand_limit(prev)


def test_conv_gemm_refuses_operands_that_are_not_dense(monkeypatch):
    """ops.conv_gemm hands data_ptr() and the shape to the library: a channel slice, a transposed map or an operand of another size
    or dtype as x, x2, residual or out would be read or written as if it were dense - EdgeStyleHipError, before anything is recorded
    or launched.  The same call with the views made contiguous goes through (dry recorder, host buffers); a time-embedding table may
    be a column slice of a wider one (es_gemm_desc.temb_stride), and a slice along the samples is dense."""
    monkeypatch.setattr(ops, "_stream", lambda: None)
    g = torch.Generator().manual_seed(0)
    N, H, W, C1, C2, Cout = 2, 6, 4, 64, 64, 128
    pw = ops.pack_weight(torch.randn(Cout, C1 + C2, 3, 3, generator=g), torch.randn(Cout, generator=g), torch.float16, "cpu")
    wide_x = torch.randn(N, H, W, 2 * C1, generator=g).half()
    wide_o = torch.zeros(N, H, W, 2 * Cout).half()
    x, x2 = torch.randn(N, H, W, C1, generator=g).half(), torch.randn(N, H, W, C2, generator=g).half()
    res, temb = torch.randn(N, H, W, Cout, generator=g).half(), torch.randn(N, Cout + 64, generator=g).half()
    bad = [dict(x=wide_x[..., :C1]), dict(x=torch.randn(N, W, H, C1, generator=g).half().transpose(1, 2)), dict(x2=wide_x[..., C1:]),
           dict(residual=wide_o[..., :Cout]), dict(out=wide_o[..., Cout:]), dict(residual=res[:1]), dict(out=torch.zeros(N, H, W, Cout)),
           dict(x2=torch.randn(N, H, W + 1, C2, generator=g).half()[:, :, :W])]
    with _DryPlan() as dry:
        for kw in bad:
            a = dict(x=x, x2=x2, residual=res, out=None, temb=temb[:, 64:])
            a.update(kw)
            with pytest.raises(lib.EdgeStyleHipError, match="conv_gemm: (x|x2|residual|out) "):
                ops.conv_gemm(a.pop("x"), pw, splitk=1, **a)
            assert dry.size() == 0, kw
        y = ops.conv_gemm(wide_x[..., :C1].contiguous(), pw, x2=wide_x[..., C1:].contiguous(), residual=wide_o[..., :Cout].contiguous(),
                          temb=temb[:, 64:], splitk=1)
        assert dry.size() == 1 and y.shape == (N, H, W, Cout)
        ops.conv_gemm(x[1:], pw, x2=x2[1:], residual=res[1:], out=wide_o.reshape(2 * N, H, W, Cout)[1:2], splitk=1)
        assert dry.size() == 2


def test_fusion_block_refuses_operands_the_launch_cannot_read(monkeypatch):
    """ops.fusion_block / ops.fusion_blocks hand data_ptr()s, N, HW, C and six batch strides to the library: a residual or a parameter of
    another dtype, a residual that is not dense inside a sample, a batch stride below HW C (or another than the view's), a view with
    fewer samples than the launch reads, affine planes packed for another size, parameter vectors of another length, an `out` that is
    not a contiguous [N, HW, C] and a short scales_dev - EdgeStyleHipError, before anything is recorded or launched (dry recorder, host
    buffers).  Views into a batched buffer - dense or with gaps between the samples - stay legal."""
    from tests import numerics as nm
    monkeypatch.setattr(ops, "_stream", lambda: None)
    N, HW, Cc = 2, 6, 16
    per = HW * Cc
    c = nm.fusion_case(N, Cc, HW, torch.float16, seed=1)
    params = {k: v.to(torch.float16 if k in ("g1", "be1", "g2", "be2") else torch.float32) for k, v in c["params"].items()}
    pose = torch.cat([c["res"][k] for k in (1, 3, 5)]).half()                                   # [3 N, HW, C], as the batched pass leaves it
    gaps = torch.zeros(N, per + 24).half()
    res = [c["res"][0].half(), pose[0:], gaps[:, :per].view(N, HW, Cc), pose[N:], c["res"][4].half().reshape(N, 2, 3, Cc), pose[2 * N:]]
    bs = [per, per, per + 24, per, per, per]
    scales = [1.0, 0.5, 1.0, 2.0, 1.0, 0.0]
    wide = torch.zeros(N, HW, 2 * Cc).half()
    other = nm.fusion_case(N, Cc, HW + 2, torch.float16, seed=1)["params"]

    def swap(i, t, stride=None):
        r, b = list(res), list(bs)
        r[i] = t
        if stride is not None:
            b[i] = stride
        return dict(res=r, res_bs=b)

    def par(**kw):
        p = dict(params)
        p.update(kw)
        return dict(params=p)
    bad = [swap(0, res[0].bfloat16()), swap(2, res[2].float()),                               # residual dtypes
           swap(0, wide[..., :Cc]), swap(4, torch.zeros(N, Cc, HW).half().transpose(1, 2)),    # not dense inside a sample
           swap(0, res[0], per - 8), swap(2, res[2], per),                                    # stride below HW C; not the view's stride
           swap(2, torch.zeros(N, per + 4).half()[:, :per].view(N, HW, Cc), per + 4), swap(0, torch.zeros(N * per + 4).half()[4:].view(N, HW, Cc)),   # 16-byte pieces
           swap(5, pose[2 * N + 1:]), swap(0, res[0][:1]), swap(3, torch.zeros(N, HW + 1, Cc).half()),     # too few samples; another size
           par(g1=other["g1"].half()), par(be2=other["be2"].half()), par(g2=params["g1"]),   # planes of another size
           par(be1=params["be1"].float()), par(w1=params["w1"].half()), par(b3=params["b3"].double()),    # parameter dtypes
           par(w1=params["w1"][:, :, 0].contiguous()), par(b1=params["b1"][:-1]), par(w2=params["w2"][1:]), par(b2=params["b2"][:8]),
           par(w3=params["b1"]), par(b3=torch.zeros(Cc + 8)),                                 # parameter lengths
           dict(out=wide[..., :Cc]), dict(out=torch.zeros(N, HW, Cc)), dict(out=torch.zeros(N * HW, Cc).half()), dict(out=torch.zeros(N + 1, HW, Cc).half()),
           dict(scales_dev=torch.ones(5)), dict(scales_dev=torch.ones(6).half()), dict(scales_dev=torch.ones(6, dtype=torch.float64))]
    with _DryPlan() as dry:
        for kw in bad:
            a = dict(res=res, res_bs=bs, params=params, out=None, scales_dev=None)
            a.update(kw)
            with pytest.raises(lib.EdgeStyleHipError, match="fusion_block: "):
                ops.fusion_block(a["res"], a["res_bs"], a["params"], N, HW, Cc, scales, a["scales_dev"], out=a["out"])
            assert dry.size() == 0, kw
            blocks = [(res, bs, params, HW, Cc)] * 13 + [(a["res"], a["res_bs"], a["params"], HW, Cc)]
            if a["out"] is None:                # the 14th block is refused before the first 13 are recorded
                with pytest.raises(lib.EdgeStyleHipError, match="fusion_block: "):
                    ops.fusion_blocks(blocks, N, scales, a["scales_dev"])
                assert dry.size() == 0, kw
        with pytest.raises(lib.EdgeStyleHipError, match="fusion_block: addend"):
            ops.fusion_blocks([(res, bs, params, HW, Cc)], N, scales, addends=[wide[..., :Cc]])
        assert dry.size() == 0
        out = torch.zeros(N + 2, HW, Cc).half()
        y = ops.fusion_block(res, bs, params, N, HW, Cc, scales, torch.ones(6), out=out[1:N + 1])
        assert dry.size() == 1 and y.data_ptr() == out[1].data_ptr()
        outs = ops.fusion_blocks([(res, bs, params, HW, Cc)] * 3, N, scales, addends=[torch.zeros(N, HW, Cc).half()] * 3)
        assert dry.size() == 2 and len(outs) == 3 and outs[0].shape == (N, HW, Cc)


def test_attention_refuses_operands_the_launch_cannot_read(monkeypatch):
    """ops.attention hands data_ptr()s, one (N, heads, Sq, Skv, d) and row / batch strides to the library: k / v / out of another dtype,
    N, width or length than that launch reads, a width that is no multiple of heads, a view whose address, row stride or batch stride
    is not a whole number of 16-byte vectors (out: of 8-byte pieces) or whose rows overlap - EdgeStyleHipError, before anything is
    recorded or launched (dry recorder, host buffers).  Column slices of a fused buffer, batch slices and a strided `out` stay legal.
    es_attention itself refuses k / v whose 32-bit buffer range or tile offsets would pass 2^31."""
    monkeypatch.setattr(ops, "_stream", lambda: None)
    N, heads, Sq, Skv, Cc = 2, 2, 6, 5, 80
    z = lambda *s: torch.zeros(*s).half()
    q, k, v = z(N, Sq, Cc), z(N, Skv, Cc), z(N, Skv, Cc)
    fused = z(N, Skv + 3, 3 * Cc + 24)
    bad = {
        "q must be fp16 or bf16": dict(q=q.float(), k=k.float(), v=v.float()),
        "q, k, v must be .N, S, heads . d.": dict(q=q[0]),
        "k is torch.bfloat16": dict(k=k.bfloat16()),
        "v is torch.float32": dict(v=v.float()),
        "out is torch.bfloat16": dict(out=q.bfloat16()),
        "k is torch.float16 on meta": dict(k=k.to("meta")),
        "k .* and v .* differ": dict(v=z(N, Skv + 1, Cc)),
        "k / v .* do not match q .* in N or width": dict(k=z(N + 1, Skv, Cc), v=z(N + 1, Skv, Cc)),
        "k / v .* do not match q .* in N or width#": dict(k=z(N, Skv, Cc + 8), v=z(N, Skv, Cc + 8)),
        "width 80 is not a multiple of heads 3": dict(heads=3),
        "out .* is not q's shape": dict(out=z(N, Sq + 1, Cc)),
        "out .* is not q's shape#": dict(out=z(N * Sq, Cc)),
        "innermost stride must be 1": dict(q=z(N, Cc, Sq).transpose(1, 2)),
        "q: row stride 40 below the width 80": dict(q=torch.as_strided(z(4096), (N, Sq, Cc), (Sq * Cc, 40, 1))),
        "k: row stride, batch stride and address must be multiples of 16 bytes": dict(k=z(N, Skv, Cc + 4)[..., :Cc]),
        "v: row stride, batch stride and address must be multiples of 16 bytes": dict(v=z(N, Skv * Cc + 4)[:, :Skv * Cc].view(N, Skv, Cc)),
        "q: row stride, batch stride and address must be multiples of 16 bytes": dict(q=z(N * Sq * Cc + 4)[4:].view(N, Sq, Cc)),
        "out: row stride, batch stride and address must be multiples of 8 bytes": dict(out=z(N, Sq, Cc + 2)[..., :Cc]),
        "out: row stride, batch stride and address must be multiples of 8 bytes#": dict(out=z(N * Sq * Cc + 2)[2:].view(N, Sq, Cc)),
    }
    with _DryPlan() as dry:
        for msg, kw in bad.items():
            a = dict(q=q, k=k, v=v, heads=heads, out=None)
            a.update(kw)
            with pytest.raises(lib.EdgeStyleHipError, match="attention: " + msg.rstrip("#")):
                ops.attention(a["q"], a["k"], a["v"], a["heads"], out=a["out"])
            assert dry.size() == 0, msg
        y = ops.attention(q, k, v, heads)
        assert dry.size() == 1 and y.shape == q.shape and y.is_contiguous()
        # q | k | v as column slices of one fused projection (with padding columns), batch slices, an `out` with padded rows and samples
        ops.attention(fused[:, :Sq - 2, :Cc], fused[:, :, Cc + 8:2 * Cc + 8], fused[:, :, 2 * Cc + 16:3 * Cc + 16], heads)
        assert dry.size() == 2
        big, outb = z(N + 2, Sq, Cc), z(N + 1, Sq + 3, Cc + 4)
        y = ops.attention(big[1:N + 1], k, v, heads, out=outb[1:, 2:Sq + 2, :Cc])
        assert dry.size() == 3 and y.data_ptr() == outb[1, 2].data_ptr()
        ops.attention(torch.as_strided(z(128), (1, 1, Cc), (3, Cc, 1)), k[:1], v[:1], heads)      # one sample: its batch stride is never used
        assert dry.size() == 4

        # the library's own limit: ((Skv - 1) * ld + d) * 2 and (Skv + 2 * 64) * ld * 2 must fit in 31 bits, for k and for v
        L = dry.L
        hostbuf = (ctypes.c_char * 4096)()

        def desc(**kw):
            d = lib.AttnDesc()
            d.q = d.k = d.v = d.o = ctypes.addressof(hostbuf)
            d.N, d.heads, d.Sq, d.Skv, d.d = 1, 1, 64, 4096, 40
            d.ldq = d.ldk = d.ldv = d.ldo = 40
            d.bsq = d.bsk = d.bsv = d.bso = 0
            d.scale, d.dtype = 1.0, lib.ES_F16
            for name, val in kw.items():
                setattr(d, name, val)
            return d
        assert L.es_attention(ctypes.byref(desc()), None) == 0 and dry.size() == 5
        edge = (1 << 30) // (4096 + 128)                    # the largest row stride (elements) whose tile offsets stay below 2^31 ...
        edge -= edge % 8
        assert (4096 + 128) * edge * 2 < 1 << 31 <= (4096 + 128) * (edge + 8) * 2
        assert L.es_attention(ctypes.byref(desc(ldk=edge, ldv=edge)), None) == 0 and dry.size() == 6
        for kw in (dict(ldk=edge + 8), dict(ldv=edge + 8), dict(Skv=1 << 26), dict(Skv=(1 << 31) - 1, ldk=8, ldv=8, d=8)):
            assert L.es_attention(ctypes.byref(desc(**kw)), None) == -1, kw
            assert b"es_attention: k / v too long for 32-bit buffer offsets" in L.es_last_error(), (kw, L.es_last_error())
            assert dry.size() == 6, kw
        assert L.es_attention(ctypes.byref(desc(ldk=32)), None) == -1 and b"row stride below head_dim" in L.es_last_error()
        assert dry.size() == 6


def _attn_knobs(**kw):
    k = lib.AttnKnobs()
    for name, val in kw.items():
        setattr(k, name, val)
    return k


def _own_attn_knobs_are_the_defaults():
    """the knobs of this process against the documented defaults; with an ES_ATTN_* variable set, nothing is asserted (and why is printed)"""
    from tests import numerics as nm
    own = lib.AttnKnobs()
    lib.load().es_attention_knobs(own)
    own = {name: getattr(own, name) for name in nm.ATTN_KNOBS}
    set_here = sorted(v for v in ("ES_ATTN_KVRES", "ES_ATTN_BIG", "ES_ATTN32", "ES_ATTN_QB", "ES_ATTN_PP") if v in os.environ)
    if set_here:
        print(f"attention knobs: {set_here} set in this process's environment - its knobs {own} are not held to the defaults")
        return False
    assert own == nm.ATTN_KNOBS == dict(kvres=1, big_thr=512, attn32=1, qb=2, pp=-1), own
    return True


def test_attention_route_is_the_mirrors_answer_under_every_knob():
    """es_attention_route (attn_route of csrc/attention.hip, which es_attention launches from) against the Python restatement of the rules
    (tests/numerics.py attn_route) in every field, on a grid of geometries that brackets every threshold, under every setting of the five
    switches - passed in, so the process's own knobs play no part."""
    from tests import numerics as nm
    L = lib.load()
    assert lib.ATTN_ROUTE_FIELDS == nm.ATTN_ROUTE_KEYS
    a, out = lib.AttnDesc(), (ctypes.c_int32 * len(lib.ATTN_ROUTE_FIELDS))()
    knob_grid = [dict(kvres=kv, attn32=a32, pp=pp, qb=qb, big_thr=big)
                 for kv in (0, 1, 2) for a32 in (0, 1, 2) for pp in (-1, 0, 1, 2) for qb in (1, 2) for big in (1, 512)]
    knob_grid = [(k, _attn_knobs(**k)) for k in knob_grid]
    kernels = set()
    for N, heads in [(1, 1), (2, 8), (11, 1), (12, 1), (63, 1), (64, 1), (14, 8), (112, 8)]:
        for d in nm.ATTN_WIDTHS:
            for Sq in (1, 63, 64, 65, 127, 129, 255, 257, 4096):
                for Skv in (1, 64, 77, 96, 97, 127, 128, 192, 4096):
                    a.N, a.heads, a.Sq, a.Skv, a.d = N, heads, Sq, Skv, d
                    a.ldq = a.ldk = a.ldv = a.ldo = heads * d
                    for k, ck in knob_grid:
                        assert L.es_attention_route(ctypes.byref(a), ctypes.byref(ck), out) == 0, (N, heads, Sq, Skv, d, L.es_last_error())
                        want = nm.attn_route(N, heads, Sq, Skv, d, k)
                        assert tuple(out) == tuple(want[f] for f in lib.ATTN_ROUTE_FIELDS), (N, heads, Sq, Skv, d, k, list(out), want)
                        kernels.add(out[0])
    assert kernels == {1, 2, 3, 4, 5, 6, 7}
    # the helper and a NULL knobs pointer: the process's own knobs
    own = lib.AttnKnobs()
    L.es_attention_knobs(own)
    own = {name: getattr(own, name) for name in nm.ATTN_KNOBS}
    for shape in [(14, 8, 4096, 77, 40), (2, 8, 4096, 4096, 40), (2, 8, 1024, 1024, 80)]:
        assert lib.attention_route(*shape) == nm.attn_route(*shape, own)
        assert lib.attention_route(*shape, knobs=_attn_knobs(**dict(nm.ATTN_KNOBS, kvres=0))) == nm.attn_route(*shape, dict(nm.ATTN_KNOBS, kvres=0))


def test_attention_knobs_default_and_follow_set_kvres():
    """es_attention_knobs returns the documented defaults (ES_ATTN_* unset here), and es_attention_set_kvres edits that struct"""
    L = lib.load()
    _own_attn_knobs_are_the_defaults()
    k = lib.AttnKnobs()
    L.es_attention_knobs(k)
    first = k.kvres
    assert L.es_attention_set_kvres(2) == first
    try:
        L.es_attention_knobs(k)
        assert k.kvres == 2 and lib.attention_route(2, 8, 4096, 77, 40)["kernel"] == 7
        assert L.es_attention_set_kvres(0) == 2 and lib.attention_route(14, 8, 4096, 77, 40)["kernel"] != 7
    finally:
        L.es_attention_set_kvres(first)
    L.es_attention_knobs(k)
    assert k.kvres == first


def test_attention_production_dispatch_table():
    """Which kernel, on which grid, every attention launch of a 512 x 512 step goes to under default knobs, as both hosts issue them: 14
    samples (batch 1: the grouped encoder pass) and 2 (the decoder), 112 and 16 at batch 8; self-attention at 64^2 / 32^2 / 16^2 / 8^2 tokens
    with 8 heads of 40 / 80 / 160 / 160, the text cross-attention (77 keys) at the same levels, and the VAE's one head of 512 over 4096
    tokens.  The literals are worked out from the rules in the header of csrc/attention.hip's host section, not read off the library;
    DESIGN section 4 names the same choices: the ping-pong kernel (5) for the level-0 self-attention, K/V-resident (7) from 14 samples at
    head_dim 40 and from 112 at head_dim 80, tiled kernels for the 2-sample decoder's cross-attention."""
    if not _own_attn_knobs_are_the_defaults():
        return
    levels = [(4096, 40), (1024, 80), (256, 160), (64, 160)]
    # self-attention: (kernel, grid x, threads) per level; grid y = 8 heads, grid z = N
    self_attn = {
        14: [(5, 16, 512), (2, 8, 256), (1, 2, 256), (1, 1, 256)],
        2: [(5, 16, 512), (1, 16, 256), (1, 2, 256), (1, 1, 256)],          # 16 x 8 x 2 = 256 workgroups of 256 queries: still the ping-pong kernel
        112: [(5, 16, 512), (2, 8, 256), (1, 2, 256), (1, 1, 256)],
        16: [(5, 16, 512), (2, 8, 256), (1, 2, 256), (1, 1, 256)],
    }
    # cross-attention, 77 keys: (kernel, grid x, grid y, threads, queries per strip)
    cross_attn = {
        14: [(7, 16, 1, 512, 256), (2, 8, 8, 256, 0), (1, 2, 8, 256, 0), (1, 1, 8, 256, 0)],
        2: [(3, 32, 8, 256, 0), (1, 16, 8, 256, 0), (1, 2, 8, 256, 0), (1, 1, 8, 256, 0)],
        112: [(7, 2, 1, 512, 2048), (7, 2, 1, 512, 512), (1, 2, 8, 256, 0), (1, 1, 8, 256, 0)],
        16: [(7, 16, 1, 512, 256), (2, 8, 8, 256, 0), (1, 2, 8, 256, 0), (1, 1, 8, 256, 0)],
    }
    for N in (14, 2, 112, 16):
        for (S, d), (kernel, gx, threads), (xkernel, xgx, xgy, xthreads, qper) in zip(levels, self_attn[N], cross_attn[N]):
            r = lib.attention_route(N, 8, S, S, d)
            assert (r["kernel"], r["grid_x"], r["grid_y"], r["grid_z"], r["threads"], r["qper"]) == (kernel, gx, 8, N, threads, 0), (N, S, d, r)
            r = lib.attention_route(N, 8, S, 77, d)
            assert (r["kernel"], r["grid_x"], r["grid_y"], r["grid_z"], r["threads"], r["qper"]) == (xkernel, xgx, xgy, N, xthreads, qper), (N, S, d, r)
    for N in (1, 8):        # the VAE's mid-block attention: 16 queries per wave, one K/V buffer of 32 keys
        r = lib.attention_route(N, 1, 4096, 4096, 512)
        assert (r["kernel"], r["q_per_wave"], r["grid_x"], r["grid_y"], r["grid_z"], r["threads"]) == (1, 16, 64, 1, N, 256), r
        assert r["lds"] == 32 * (1024 + 16) + 32 * (1024 + 16)


def test_attention_route_refuses_what_the_launch_refuses():
    """es_attention_route and es_attention (dry recorder, host buffers) refuse the same geometries with the same texts - an unsupported
    head_dim, strides that are no multiples of 8 or below head_dim, an empty problem, a K/V range past 2^31 - and the query reads no
    pointer: NULL ones are fine."""
    out = (ctypes.c_int32 * len(lib.ATTN_ROUTE_FIELDS))()
    hostbuf = (ctypes.c_char * 4096)()

    def desc(ptr, **kw):
        a = lib.AttnDesc()
        a.q = a.k = a.v = a.o = ptr
        a.N, a.heads, a.Sq, a.Skv, a.d = 1, 1, 64, 4096, 40
        a.ldq = a.ldk = a.ldv = a.ldo = 40
        a.scale, a.dtype = 1.0, lib.ES_F16
        for name, val in kw.items():
            setattr(a, name, val)
        return a
    refused = [(dict(d=56, ldq=56, ldk=56, ldv=56, ldo=56), b"es_attention: unsupported head_dim (8,16,24,32,40,48,64,80,128,160,512)", -3),
               (dict(d=44), b"es_attention: d and strides must be multiples of 8", -1),
               (dict(ldk=44), b"es_attention: d and strides must be multiples of 8", -1),
               (dict(ldk=32), b"es_attention: a k / v row stride below head_dim", -1),
               (dict(ldv=32), b"es_attention: a k / v row stride below head_dim", -1),
               (dict(Sq=0), b"es_attention: empty problem", -1), (dict(Skv=0), b"es_attention: empty problem", -1),
               (dict(N=0), b"es_attention: empty problem", -1), (dict(heads=0), b"es_attention: empty problem", -1),
               (dict(Skv=1 << 26), b"es_attention: k / v too long for 32-bit buffer offsets ((Skv + 128) * ld * 2 must stay below 2^31)", -1),
               (dict(ldv=(1 << 30) // (4096 + 128) + 8), b"es_attention: k / v too long for 32-bit buffer offsets ((Skv + 128) * ld * 2 must stay below 2^31)", -1)]
    with _DryPlan() as dry:
        L = dry.L
        assert L.es_attention_route(ctypes.byref(desc(None)), None, out) == 0 and out[0] != 0
        assert L.es_attention(ctypes.byref(desc(None)), None) == -1 and L.es_last_error() == b"es_attention: null pointer"
        assert L.es_attention(ctypes.byref(desc(ctypes.addressof(hostbuf))), None) == 0 and dry.size() == 1
        for kw, text, rc in refused:
            assert L.es_attention_route(ctypes.byref(desc(None, **kw)), None, out) == -1 and L.es_last_error() == text, (kw, L.es_last_error())
            assert L.es_attention(ctypes.byref(desc(ctypes.addressof(hostbuf), **kw)), None) == rc and L.es_last_error() == text, (kw, L.es_last_error())
            assert dry.size() == 1, kw
        with pytest.raises(lib.EdgeStyleHipError, match="unsupported head_dim"):
            lib.attention_route(1, 1, 64, 64, 56)
        assert dry.size() == 1              # the query records nothing


def test_attention_route_states_the_geometry_the_kernel_id_leaves_open():
    """Kernel id 1 ("generic, 16 queries per wave") is also what head widths 8-32, 64, 128 and 160 report, which always run 32 queries per
    wave: the route says which.  Default knobs, a launch far below the 512-block threshold."""
    if not _own_attn_knobs_are_the_defaults():
        return
    r64, r40 = lib.attention_route(1, 1, 70, 77, 64), lib.attention_route(1, 1, 70, 77, 40)
    assert (r64["kernel"], r64["q_per_wave"], r64["q_per_wg"], r64["grid_x"]) == (1, 32, 128, 1), r64
    assert (r40["kernel"], r40["q_per_wave"], r40["q_per_wg"], r40["grid_x"]) == (1, 16, 64, 2), r40


def _gn_two_launch_route(HW):
    """groups of ONE channel are never eligible for the slab form: the statistics pass's own geometry for this HW"""
    r = lib.group_norm_route(1, HW, 8, 0, 8)
    assert r["form"] == lib.GN_FORM_TWO_LAUNCHES
    return r


def test_group_norm_chunks_fit_the_partials_buffer_for_every_size():
    """The statistics pass writes es_group_norm_chunks(HW) rows of `partials` per sample and both hosts allocate 64
    (es_group_norm_partials_bytes): 1 <= chunks <= 64 for EVERY HW, the chunks cover HW with none of them empty, and the sizes the models
    and the goldens use keep the chunking they had.  With the chunk size rounded DOWN (max(16, HW / 64)) every HW > 1024 that is no multiple
    of 64 gave 65 .. 68 chunks - first at HW = 1025 - and the two launches wrote and read up to N * 4 * groups * 2 floats behind the buffer."""
    L = lib.load()
    sizes = list(range(1, 70001)) + [70001 + 7919 * k for k in range(1, 64)] + [(1 << 20) - 1, (1 << 20) + 1, (1 << 24) - 65, (1 << 24) - 1, 1 << 24]
    for HW in sizes:
        n = L.es_group_norm_chunks(HW)
        assert 1 <= n <= 64, (HW, n)
        if HW <= 2048 or HW % 997 == 0 or HW > 70000:       # the route query is the launcher's own code: same chunk count, and its chunk size covers HW
            r = _gn_two_launch_route(HW)
            assert r["nchunk"] == n and r["ppb"] >= 16 and (n - 1) * r["ppb"] < HW <= n * r["ppb"], (HW, r)
        ppb = max(16, -(-HW // 64))
        assert (n - 1) * ppb < HW <= n * ppb, (HW, n)
    for HW, n in {16: 1, 64: 4, 144: 9, 256: 16, 1023: 64, 1024: 64, 4096: 64, 9216: 64, 65536: 64}.items():       # read off the commit before the fix
        assert L.es_group_norm_chunks(HW) == n, HW
    for HW, ppb in {1023: 16, 1024: 16, 1025: 17, 4096: 64, 9216: 144}.items():
        assert _gn_two_launch_route(HW)["ppb"] == ppb
    assert L.es_group_norm_chunks(0) == 0
    for N, G in [(1, 1), (3, 32), (14, 64)]:
        assert L.es_group_norm_partials_bytes(N, G) == N * 64 * G * 2 * 4
    from tests import numerics as nm
    for HW in (1, 15, 16, 17, 1023, 1025, 1087, 1225, 1296, 4225, 69999):
        assert nm.gn_pixels_per_chunk(HW) == _gn_two_launch_route(HW)["ppb"]


def test_group_norm_route_is_the_launchers_own_answer():
    """es_group_norm_route / es_layer_norm_route against the Python mirror of the rule (tests/numerics.py gn_route) on a grid of geometries, the
    form against es_group_norm_is_slab, and the refusals the launch itself would make."""
    from tests import numerics as nm
    L = lib.load()
    for HW in (1, 7, 24, 25, 64, 408, 409, 816, 817, 1224, 1225, 4096, 9216):
        for Cc, G in [(8, 1), (8, 8), (24, 8), (64, 64), (120, 40), (128, 64), (320, 32), (640, 32), (1040, 8), (1280, 32), (2048, 1), (2056, 1), (2560, 32)]:
            for N in (1, 3, 14):
                r = lib.group_norm_route(N, HW, Cc, 0, G)
                assert r == nm.gn_route(N, HW, Cc, G), (N, HW, Cc, G, r)
                assert (r["form"] == lib.GN_FORM_SLAB) == bool(L.es_group_norm_is_slab(HW, Cc, G))
            s = lib.group_norm_route(3, HW, Cc, 0, G, stats_only=True)
            assert s == nm.gn_route(3, HW, Cc, G, stats_only=True) and s["form"] == lib.GN_FORM_TWO_LAUNCHES and s["blocks"] == 0
            assert s["nchunk"] == L.es_group_norm_chunks(HW)
    r = lib.group_norm_route(2, 4096, 320, 0, 32, ext_chunks=128)          # the producer's statistics: 2 * HW / 64 rows, no slab
    assert r["form"] == lib.GN_FORM_TWO_LAUNCHES and r["nchunk"] == 128
    assert lib.group_norm_route(2, 64, 1280, 0, 32)["form"] == lib.GN_FORM_SLAB
    assert lib.group_norm_route(14, 4096, 320, 0, 32)["ipt"] == 8 and lib.group_norm_route(2, 4096, 320, 0, 32)["ipt"] == 4
    for kw, msg in [(dict(C1=12), "multiples of 8"), (dict(groups=3), "bad group count"), (dict(groups=65, C1=520), "bad group count"),
                    (dict(HW=0), "empty problem"), (dict(C1=8200, groups=1), "C too large")]:
        a = dict(N=1, HW=64, C1=320, C2=0, groups=32)
        a.update(kw)
        with pytest.raises(lib.EdgeStyleHipError, match=msg):
            lib.group_norm_route(**a)
    for Cc, vpl in {8: 1, 512: 1, 520: 2, 1024: 2, 1032: 3, 1536: 3, 1544: 4, 2048: 4, 2056: 8, 4096: 8, 4104: 0, 12: 0, 0: 0}.items():
        assert L.es_layer_norm_route(Cc) == vpl, Cc


def test_group_norm_refuses_tables_that_do_not_fit_the_lds():
    """gn_apply_kernel keeps (2 C + 2 groups + 256) floats in dynamic LDS and a launch gets 64 KB: a two-launch geometry with
    C + groups > 8064 is refused by name, before it is recorded (dry recorder, host buffers) - not left to fail as a launch error.  The slab
    form and the statistics pass alone need less and stay legal up to C = 8192; so does LayerNorm's limit of 4096 channels."""
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)

    def desc(Cc, G, HW=4096, **kw):
        d = lib.GnDesc()
        d.x = d.out = d.gamma = d.beta = d.partials = p
        d.N, d.HW, d.C1, d.C2, d.groups, d.eps, d.dtype = 2, HW, Cc, 0, G, 1e-5, lib.ES_F16
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    with _DryPlan() as dry:
        L = dry.L
        assert L.es_group_norm(ctypes.byref(desc(8000, 32)), None) == 0 and dry.size() == 1            # 65 280 bytes
        assert L.es_group_norm(ctypes.byref(desc(8056, 8)), None) == 0 and dry.size() == 2             # 65 536 bytes: the limit itself
        for Cc, G in [(8064, 1), (8064, 64), (8192, 1), (8056, 19)]:
            assert lib.group_norm_route(2, 4096, Cc, 0, G, stats_only=True)["form"] == lib.GN_FORM_TWO_LAUNCHES
            assert L.es_group_norm(ctypes.byref(desc(Cc, G)), None) == -1, (Cc, G)
            assert b"es_group_norm: the two-launch form's scale / shift tables exceed 64 KB of LDS" in L.es_last_error(), L.es_last_error()
            with pytest.raises(lib.EdgeStyleHipError, match="64 KB of LDS"):
                lib.group_norm_route(2, 4096, Cc, 0, G)
            assert dry.size() == 2
        assert L.es_group_norm(ctypes.byref(desc(8192, 1, stats_only=1)), None) == 0 and dry.size() == 3      # the statistics pass alone: 64 KB
        assert lib.group_norm_route(2, 16, 8192, 0, 64)["form"] == lib.GN_FORM_SLAB
        assert L.es_group_norm(ctypes.byref(desc(8192, 64, HW=16)), None) == 0 and dry.size() == 4            # slab: 16 KB
        assert L.es_group_norm(ctypes.byref(desc(8200, 1)), None) == -1 and b"C too large" in L.es_last_error()
        assert L.es_layer_norm(p, p, p, p, 4, 4096, 1e-5, lib.ES_F16, None) == 0 and dry.size() == 5
        assert L.es_layer_norm(p, p, p, p, 4, 4104, 1e-5, lib.ES_F16, None) == -1 and b"C > 4096 unsupported" in L.es_last_error()
        ln = lib.LnDesc()
        ln.x = ln.out = p
        ln.ngroups, ln.M, ln.C, ln.eps, ln.dtype = 2, 8, 4104, 1e-5, lib.ES_F16
        for g in range(2):
            ln.gamma_g[g] = ln.beta_g[g] = p
            ln.row_end[g] = 4 * (g + 1)
        assert L.es_layer_norm_grouped(ctypes.byref(ln), None) == -1 and b"C > 4096 unsupported" in L.es_last_error()
        assert dry.size() == 5


def test_norm_wrappers_refuse_operands_the_launch_cannot_read(monkeypatch):
    """ops.group_norm, ops.gn_proj_in and ops.layer_norm hand data_ptr()s and one geometry to the library, which reads every operand as dense:
    a non-contiguous x or x2, x2 of another dtype, device or N, H, W, channel counts that are no multiples of 8 or do not divide into the
    groups, gamma / beta that are not fp32, not C long or elsewhere, an `out` or `partials` of another shape, and any of x, x2, out, gamma,
    beta that does not start at a multiple of 16 bytes (all are read or written as 16-byte vectors) - EdgeStyleHipError by name,
    before anything is recorded or launched (dry recorder, host buffers).  Batch slices and out= / partials= of the right shape stay legal."""
    monkeypatch.setattr(ops, "_stream", lambda: None)
    N, H, W, C1, C2, G = 2, 3, 5, 16, 24, 8
    z = lambda *s: torch.zeros(*s).half()
    x, x2 = z(N, H, W, C1), z(N, H, W, C2)
    f = lambda n: torch.ones(n)
    gn_bad = {
        "x must be contiguous": dict(x=z(N, H, W, 2 * C1)[..., :C1]),
        "x must be contiguous#": dict(x=z(N, W, H, C1).transpose(1, 2)),
        "x must be an fp16 or bf16": dict(x=x.float()),
        "x must be an fp16 or bf16#": dict(x=x[0]),
        "x2 must be contiguous": dict(x2=z(N, H, W, 2 * C2)[..., C2:]),
        "x2 is torch.bfloat16": dict(x2=x2.bfloat16()),
        "x2 is torch.float16 on meta": dict(x2=x2.to("meta")),
        "x2 .* does not match x .* in N, H, W": dict(x2=z(N, H, W + 1, C2)),
        "x2 .* does not match x .* in N, H, W#": dict(x2=z(N + 1, H, W, C2)[:N + 1]),
        "channels 12.24 must be multiples of 8": dict(x=z(N, H, W, 12), gamma=f(36), beta=f(36), groups=4),
        "channels 16.20 must be multiples of 8": dict(x2=z(N, H, W, 20), gamma=f(36), beta=f(36), groups=4),
        "40 channels do not divide into 7 groups": dict(groups=7),
        "gamma must be a contiguous fp32 .40. tensor": dict(gamma=f(40).half()),
        "gamma must be a contiguous fp32 .40. tensor#": dict(gamma=f(32)),
        "gamma must be a contiguous fp32 .40. tensor##": dict(gamma=f(80)[::2]),
        "beta must be a contiguous fp32 .40. tensor": dict(beta=f(40).double()),
        "beta must be a contiguous fp32 .40. tensor#": dict(beta=f(48)),
        "beta must be a contiguous fp32 .40. tensor on cpu": dict(beta=f(40).to("meta")),
        "gamma must start at a multiple of 16 bytes": dict(gamma=f(41)[1:]),
        "beta must start at a multiple of 16 bytes": dict(beta=f(42)[2:]),
        "x must start at a multiple of 16 bytes": dict(x=z(N * H * W * C1 + 4)[4:].view(N, H, W, C1)),
        "x2 must start at a multiple of 16 bytes": dict(x2=z(N * H * W * C2 + 4)[4:].view(N, H, W, C2)),
        "out must start at a multiple of 16 bytes": dict(out=z(N * H * W * 40 + 4)[4:].view(N, H, W, 40)),
        "bad group table": dict(gamma=[f(40), f(40)], beta=[f(40), f(40)], group_n=[1, 2]),
        "2 gamma and 1 beta sets": dict(gamma=[f(40), f(40)], beta=[f(40)], group_n=[1, 1]),
        "out must be a contiguous torch.float16 .2, 3, 5, 40.": dict(out=z(N, H, W, C1)),
        "out must be a contiguous torch.float16 .2, 3, 5, 40.#": dict(out=z(N, H, W, 80)[..., :40]),
        "out must be a contiguous torch.float16 .2, 3, 5, 40.##": dict(out=torch.zeros(N, H, W, 40)),
        "out must be a contiguous torch.float16 .2, 3, 5, 40.###": dict(out=z(N * H * W, 40)),
        "partials must be a contiguous fp32 tensor of 2048 elements": dict(partials=torch.zeros(N * 32 * G * 2)),
        "partials must be a contiguous fp32 tensor of 2048 elements#": dict(partials=torch.zeros(2048).half()),
        "partials must be a contiguous fp32 tensor of 2048 elements##": dict(partials=torch.zeros(4096)[::2]),
    }
    with _DryPlan() as dry:
        for msg, kw in gn_bad.items():
            a = dict(x=x, x2=x2, gamma=f(40), beta=f(40), groups=G, group_n=None, out=None, partials=None)
            a.update(kw)
            with pytest.raises(lib.EdgeStyleHipError, match="group_norm: " + msg.rstrip("#")):
                ops.group_norm(a["x"], a["gamma"], a["beta"], a["groups"], 1e-5, True, x2=a["x2"], group_n=a["group_n"], out=a["out"], partials=a["partials"])
            assert dry.size() == 0, msg
        out, part = z(N + 2, H, W, 40), torch.zeros(3 * 2048)
        y = ops.group_norm(x, f(40), f(40), G, 1e-5, True, x2=x2, out=out[1:N + 1], partials=part[2048:4096])
        assert dry.size() == 1 and y.data_ptr() == out[1].data_ptr()
        y = ops.group_norm(z(N + 1, H, W, C1)[1:], [f(40), f(40)], [f(40), f(40)], G, 1e-5, False, x2=x2, group_n=[1, 1])
        assert dry.size() == 2 and y.shape == (N, H, W, 40) and y.is_contiguous()

        # gn_proj_in: the same demands on x, gamma and beta, whichever form runs
        g = torch.Generator().manual_seed(0)
        pw = ops.pack_weight(torch.randn(64, 40, 1, 1, generator=g), torch.randn(64, generator=g), torch.float16, "cpu")
        xin = z(N, H, W, 40)
        proj_bad = {
            "x must be contiguous": dict(x=z(N, H, W, 80)[..., :40]),
            "x must be an fp16 or bf16": dict(x=xin.float()),
            "40 channels do not divide into 7 groups": dict(groups=7),
            "gamma must be a contiguous fp32 .40. tensor": dict(gamma=f(40).half()),
            "beta must be a contiguous fp32 .40. tensor": dict(beta=f(32)),
            "channels 36.0 must be multiples of 8": dict(x=z(N, H, W, 36), gamma=f(36), beta=f(36), groups=4),
        }
        for msg, kw in proj_bad.items():
            a = dict(x=xin, gamma=f(40), beta=f(40), groups=G)
            a.update(kw)
            with pytest.raises(lib.EdgeStyleHipError, match="gn_proj_in: " + msg):
                ops.gn_proj_in(a["x"], a["gamma"], a["beta"], a["groups"], 1e-6, pw)
            assert dry.size() == 2, msg
        y = ops.gn_proj_in(xin, f(40), f(40), G, 1e-6, pw)
        assert dry.size() == 4 and y.shape == (N, H, W, 64)              # GroupNorm + projection

        tok = z(6, 40)
        ln_bad = {
            "x must be contiguous": dict(x=z(6, 80)[:, :40]),
            "x must be contiguous, not empty and C a multiple of 8": dict(x=z(6, 36), gamma=f(36), beta=f(36)),
            "x must be an fp16 or bf16": dict(x=tok.float()),
            "gamma must be a contiguous fp32 .40. tensor": dict(gamma=f(40).bfloat16()),
            "beta must be a contiguous fp32 .40. tensor": dict(beta=f(41)),
            "beta must be a contiguous fp32 .40. tensor on cpu": dict(beta=f(40).to("meta")),
            "x must start at a multiple of 16 bytes": dict(x=z(6 * 40 + 4)[4:].view(6, 40)),
            "gamma must start at a multiple of 16 bytes": dict(gamma=f(43)[3:]),
            "out must start at a multiple of 16 bytes": dict(out=z(6 * 40 + 4)[4:].view(6, 40)),
            "bad group table": dict(gamma=[f(40)] * 2, beta=[f(40)] * 2, group_rows=[3, 4]),
            "C = 4104 > 4096 unsupported": dict(x=z(2, 4104), gamma=f(4104), beta=f(4104)),
            "out must be a contiguous torch.float16 .6, 40.": dict(out=z(6, 48)),
            "out must be a contiguous torch.float16 .6, 40.#": dict(out=z(6, 80)[:, :40]),
            "out must be a contiguous torch.float16 .6, 40.##": dict(out=tok.bfloat16()),
        }
        for msg, kw in ln_bad.items():
            a = dict(x=tok, gamma=f(40), beta=f(40), group_rows=None, out=None)
            a.update(kw)
            with pytest.raises(lib.EdgeStyleHipError, match="layer_norm: " + msg.rstrip("#")):
                ops.layer_norm(a["x"], a["gamma"], a["beta"], group_rows=a["group_rows"], out=a["out"])
            assert dry.size() == 4, msg
        big = z(8, 40)
        y = ops.layer_norm(tok.view(2, 3, 40), f(40), f(40), out=big[1:7].view(2, 3, 40))
        assert dry.size() == 5 and y.data_ptr() == big[1].data_ptr()
        ops.layer_norm(tok, [f(40)] * 3, [f(40)] * 3, group_rows=[1, 4, 1])
        assert dry.size() == 6


# one refusal of ops.linear_xs per entry: message -> what to change in a legal call (M = 512 rows of K = 320 -> 128 columns, fp16)
_XS_M, _XS_K, _XS_C = 512, 320, 128
_xs_z = lambda *s: torch.zeros(*s).half()
_XS_REFUSALS = {
    "x must be fp16 or bf16": lambda a: a.update(x=a["x"].float(), out=a["out"].float()),
    "out is torch.bfloat16": lambda a: a.update(out=a["out"].bfloat16()),
    "residual is torch.float32": lambda a: a.update(residual=torch.zeros(_XS_M, _XS_C)),
    "out is torch.float16 on meta": lambda a: a.update(out=a["out"].to("meta")),
    r"x must be a contiguous \[M, K\] = \[512, 320\]": lambda a: a.update(x=_xs_z(_XS_M, 2 * _XS_K)[:, :_XS_K]),
    r"x must be a contiguous \[M, K\] = \[512, 320\]#": lambda a: a.update(x=_xs_z(_XS_M, 1, 1, _XS_K)),
    r"x must be a contiguous \[M, K\] = \[512, 320\]##": lambda a: a.update(x=_xs_z(_XS_M + 1, _XS_K)),
    "x must start at a multiple of 16 bytes": lambda a: a.update(x=_xs_z(_XS_M * _XS_K + 4)[4:].view(_XS_M, _XS_K)),
    r"out must be \[M, cstore\] = \[512, 128\]": lambda a: a.update(out=_xs_z(_XS_M, 1, 1, _XS_C)),
    r"out must be \[M, cstore\] = \[512, 128\]#": lambda a: a.update(out=_xs_z(_XS_M, _XS_C + 64)),
    r"residual must be \[M, cstore\] = \[512, 128\]": lambda a: a.update(residual=_xs_z(_XS_M, 1, 1, _XS_C)),
    "out: innermost stride must be 1": lambda a: a.update(out=_xs_z(_XS_C, _XS_M).t()),
    "residual: innermost stride must be 1": lambda a: a.update(residual=_xs_z(_XS_C, _XS_M).t()),
    "out: row pitch 132 must be a multiple of 8 elements": lambda a: a.update(out=_xs_z(_XS_M, _XS_C + 4)[:, :_XS_C]),
    "out: row pitch 64 must be a multiple of 8 elements and at least the width 128": lambda a: a.update(out=torch.as_strided(_xs_z(_XS_M * _XS_C), (_XS_M, _XS_C), (64, 1))),
    "residual: row pitch 128 differs from out's 192": lambda a: a.update(out=_xs_z(_XS_M, _XS_C + 64)[:, :_XS_C]),
    "out must start at a multiple of 16 bytes": lambda a: a.update(out=_xs_z(_XS_M * _XS_C + 4)[4:].view(_XS_M, _XS_C)),
    "residual must start at a multiple of 16 bytes": lambda a: a.update(residual=_xs_z(_XS_M * _XS_C + 4)[4:].view(_XS_M, _XS_C)),
    "group_rows None must hold one run of rows per weight set": lambda a: a.update(pw=[a["pw"], a["pw"]]),
    r"group_rows \[256\] must hold one run of rows per weight set": lambda a: a.update(pw=[a["pw"], a["pw"]], group_rows=[256]),
    r"group_rows \[256, 255\] must hold one run of rows per weight set and sum to M = 512": lambda a: a.update(pw=[a["pw"], a["pw"]], group_rows=[256, 255]),
    r"group_rows \[128, 384\]: every run but the last must be whole 256-row blocks": lambda a: a.update(pw=[a["pw"], a["pw"]], group_rows=[128, 384]),
}


@pytest.mark.parametrize("msg", list(_XS_REFUSALS), ids=lambda m: re.sub(r"[^A-Za-z0-9#]+", "_", m)[:60])
def test_linear_xs_wrapper_refuses_what_the_launch_cannot_address(msg, monkeypatch):
    """ops.linear_xs hands data_ptr()s, M and ONE row pitch to es_linear_xs: operands of another dtype, device, shape, inner stride,
    pitch or alignment than that launch addresses, and group tables that do not cover M in whole 256-row blocks, raise EdgeStyleHipError
    before anything is recorded or launched (dry recorder, host buffers)."""
    monkeypatch.setattr(ops, "_stream", lambda: None)
    pw = ops.pack_weight(torch.zeros(_XS_C, _XS_K), torch.zeros(_XS_C), torch.float16, "cpu")
    a = dict(x=_xs_z(_XS_M, _XS_K), pw=pw, out=_xs_z(_XS_M, _XS_C), residual=_xs_z(_XS_M, _XS_C), group_rows=None)
    _XS_REFUSALS[msg](a)
    with _DryPlan() as dry:
        with pytest.raises(lib.EdgeStyleHipError, match="linear_xs: " + msg.rstrip("#")):
            ops.linear_xs(a["x"], a["pw"], _XS_M, a["out"], a["group_rows"], residual=a["residual"])
        assert dry.size() == 0


def test_linear_xs_wrapper_passes_the_pitch_and_keeps_a_ragged_last_group(monkeypatch):
    """What stays legal: dense operands (ldo = cstore, as before), `out` and `residual` as column / row slices of ONE pitch (ldo = that
    pitch, read back from the recorded descriptor), a single row whose stride is never used - and a grouped launch whose LAST run is
    ragged, with ceil(rows / 128) odd: the choice is to SUPPORT it (mt_end of the last group = ceil(M / 128); es_linear_xs demands whole
    256-row blocks of every group but the last), while an earlier ragged run stays refused by the library as well."""
    monkeypatch.setattr(ops, "_stream", lambda: None)
    pw = ops.pack_weight(torch.zeros(_XS_C, _XS_K), torch.zeros(_XS_C), torch.float16, "cpu")
    M = _XS_M

    class Rec:
        descs = []
        next = staticmethod(lambda meta: None)
    monkeypatch.setattr(ops, "PROFILE", Rec)
    with _DryPlan() as dry:
        ops.linear_xs(_xs_z(M, _XS_K), pw, M, _xs_z(M, _XS_C), residual=_xs_z(M, _XS_C))
        assert dry.size() == 1 and Rec.descs[-1].ldo == _XS_C
        big, rbig = _xs_z(M + 8, _XS_C + 64), _xs_z(M + 2, _XS_C + 64)
        ops.linear_xs(_xs_z(M + 4, _XS_K)[2:M + 2], pw, M, big[4:M + 4, :_XS_C], residual=rbig[1:M + 1, :_XS_C])
        assert dry.size() == 2 and Rec.descs[-1].ldo == _XS_C + 64 and Rec.descs[-1].out == big[4].data_ptr()
        ops.linear_xs(_xs_z(1, _XS_K), pw, 1, torch.as_strided(_xs_z(1024), (1, _XS_C), (3, 1)))
        assert dry.size() == 3 and Rec.descs[-1].ldo == _XS_C
        # ragged last groups: 256 + 100 rows (ceil(356 / 128) = 3, odd), 512 + 256 + 1
        for rows in ([256, 100], [512, 256, 1], [256, 256]):
            m = sum(rows)
            ops.linear_xs(_xs_z(m, _XS_K), [pw] * len(rows), m, _xs_z(m, _XS_C), rows)
            d = Rec.descs[-1]
            ends = [d.mt_end[g] for g in range(len(rows))]
            assert d.ngroups == len(rows) and ends[-1] == (m + 127) // 128 and all(e % 2 == 0 for e in ends[:-1]), (rows, ends)
        assert dry.size() == 6 and [Rec.descs[-3].mt_end[g] for g in range(2)] == [2, 3]
        # the library itself: an odd boundary anywhere but at the end is refused, nothing recorded
        d = Rec.descs[-2]
        d.mt_end[0], d.mt_end[1] = 3, 6
        assert dry.L.es_linear_xs(ctypes.byref(d), None) == -1 and b"the last may be ragged" in dry.L.es_last_error() and dry.size() == 6


def test_linear_xs_last_form_is_set_by_launches_only(monkeypatch):
    """es_linear_xs_last_form: written by the launcher alone - a dry (recording) call leaves it as it was, and it is 0 in a process that
    has launched nothing (no GPU: this one); the flags are the header's"""
    monkeypatch.setattr(ops, "_stream", lambda: None)
    L = lib.load()
    before = L.es_linear_xs_last_form()
    if not torch.cuda.is_available():
        assert before == 0
    pw = ops.pack_weight(torch.zeros(_XS_C, _XS_K), torch.zeros(_XS_C), torch.float16, "cpu")
    with _DryPlan() as dry:
        ops.linear_xs(_xs_z(_XS_M, _XS_K), pw, _XS_M, _xs_z(_XS_M, _XS_C))
        assert dry.size() == 1 and L.es_linear_xs_last_form() == before
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "edgestyle_hip.h")).read()
    for name in ("GEGLU", "LN", "RES", "PP", "GN"):
        m = re.search(rf"ES_XS_FORM_{name} = (0x[0-9A-Fa-f]+)", hdr)
        assert m and int(m.group(1), 16) == getattr(lib, f"XS_FORM_{name}")


# ---- es_conv_gemm_route / es_linear_xs_route: the launch as numbers, asked on the CPU ------------------------------------------------
_HOSTBUF = (ctypes.c_char * 4096)()
_PTR = ctypes.addressof(_HOSTBUF)
_GEMM_PTRS = ("x2", "temb", "residual", "workspace", "ln_colsum", "t1", "t2", "residual_lo", "out_lo", "gn_part")


def _gemm_desc(M=128, hw=None, C1=64, C2=0, ksize=1, Cout=1280, bn=128, groups=None, **kw):
    """a descriptor es_conv_gemm accepts - M pixels as M // hw samples of hw x 1 (hw None: one sample), C1 (+ C2) -> Cout channels, host
    buffers - with `kw` laid over it: pointer fields by truth value, `groups` = the mt_end table of a grouped launch, the rest as given"""
    d = lib.GemmDesc()
    d.x = d.w = d.out = _PTR
    hw = hw or M
    d.N, d.Hout, d.Wout, d.Hsrc, d.Wsrc = M // hw, hw, 1, hw, 1
    d.C1, d.C2, d.x2 = C1, C2, _PTR if C2 else None
    d.ksize, d.stride, d.pad = ksize, 1, ksize // 2
    d.Cout, d.rows_padded = Cout, -(-Cout // bn) * bn if bn > 0 else Cout
    d.Kpad = -(-ksize * ksize * (C1 + C2) // 64) * 64
    d.splitk, d.bn, d.dtype, d.gn_groups = 1, bn, lib.ES_F16, 32
    for g, end in enumerate(groups or ()):
        d.ngroups, d.mt_end[g], d.w_g[g], d.bias_g[g] = len(groups), end, _PTR, _PTR
    for name, v in kw.items():
        setattr(d, name, (_PTR if v else None) if name in _GEMM_PTRS else v)
    return d


def _xs_desc(M=512, K=320, Cout=640, nslices=1, geglu=0, groups=None, **kw):
    d = lib.XsDesc()
    d.x = d.out = d.w = d.bias = _PTR
    ch = 64 if K == 320 else 32
    P = 128 // (ch if geglu else 2 * ch)
    d.M, d.K, d.Cout, d.rows_padded, d.geglu, d.dtype = M, K, Cout, Cout, geglu, lib.ES_F16
    d.ldo = Cout // 2 if geglu else Cout
    d.nslices, d.chunks_per_slice = nslices, -(-(-(-(Cout // ch) // nslices)) // P) * P
    d.gn_groups, d.gn_nchunk, d.gn_hw, d.gn_eps = 32, 4, 256, 1e-6
    for g, end in enumerate(groups or ()):
        d.ngroups, d.mt_end[g] = len(groups), end
        d.w_g[g] = d.bias_g[g] = d.gn_gamma_g[g] = d.gn_beta_g[g] = _PTR
    for name, v in kw.items():
        setattr(d, name, (_PTR if v else None) if name in ("residual", "gn_part", "gn_gamma", "gn_beta") else v)
    return d


def _source_texts(path, who):
    """every refusal text of `who` in a .hip file, but the two that need a pointer's target or a GPU"""
    src = open(os.path.join(ROOT, "edgestyle_amd", "csrc", path)).read()
    return {t for t in re.findall(rf'"({who}: [^"]+)"', src) if "null pointer" not in t and "launch failed" not in t}


class _RouteSweep:
    """Asks the route and a dry recording call of the entry point about each descriptor: both accept, or both refuse with one text.
    Collects the refusal texts and the routes."""

    def __init__(self, dry, route_fn, entry, fields, knobs=False):
        self.L, self.dry, self.route_fn, self.entry, self.knobs = dry.L, dry, route_fn, entry, knobs
        self.out, self.texts, self.fields = (ctypes.c_int32 * len(fields))(), set(), fields

    def ask(self, d, knobs=None):
        args = (ctypes.byref(d), knobs, self.out) if self.knobs else (ctypes.byref(d), self.out)
        rc, size = self.route_fn(*args), self.dry.size()
        if rc != 0:
            text = self.L.es_last_error()
            assert rc == -1 and self.entry(ctypes.byref(d), None) == -1 and self.L.es_last_error() == text, (text, self.L.es_last_error())
            assert self.dry.size() == size
            self.texts.add(text.decode())
            return None
        assert self.entry(ctypes.byref(d), None) == 0 and self.dry.size() == size + 1, self.L.es_last_error()
        return dict(zip(self.fields, self.out))


# one descriptor per refusal of gemm_check that the sweep below does not meet: (operand limit or 0, what to lay over _gemm_desc())
_GEMM_REFUSED = [
    (0, dict(ngroups=5)), (0, dict(ngroups=2)), (0, dict(M=256, groups=[1, 3])), (0, dict(M=256, bn=320, C1=128, ksize=3, groups=[1, 2])),
    (0, dict(bn=96)), (0, dict(bn=256, waves=8)), (0, dict(rows_padded=1284)), (0, dict(Kpad=0)), (0, dict(C1=60, Kpad=64)),
    (0, dict(C1=72, C2=64)), (0, dict(Cout=32768, Kpad=32768)), (0, dict(N=0)), (0, dict(ksize=2)),
    (1 << 20, dict(M=1024, hw=128, gn_part=1)), (1 << 15, dict(M=1024, hw=128, x_nmod=2)), (1 << 16, dict(M=1024, hw=128)),
    (1 << 20, dict(M=1024, hw=256, groups=[3, 8])), (1 << 21, dict(M=1024, hw=256, groups=[2, 8], x_nmod=2)),
    (0, dict(t1=1, Ct1=32, Kpad=128)), (0, dict(Ct1=64, Kpad=128)), (0, dict(x_nmod=2)), (0, dict(out_lo=1)), (0, dict(residual_lo=1)),
    (0, dict(gn_part=1, gn_groups=0)), (0, dict(korder=1)), (0, dict(splitk=0)), (0, dict(splitk=2, C1=128)), (0, dict(act=2, bn=160)),
    (0, dict(stages=5)), (0, dict(waves=2)), (0, dict(ln_colsum=1, ksize=3)), (0, dict(M=256, ln_colsum=1, groups=[1, 2])),
    (0, dict(waves=8, stages=3)),
]


def test_conv_gemm_route_is_the_mirrors_answer_and_refuses_what_the_launch_refuses():
    """es_conv_gemm_route (gemm_route of csrc/gemm_conv.hip, which es_conv_gemm launches from) against the Python restatement of the rules
    (tests/numerics.py gemm_route) in every field but the table row, over two hand-pruned grids: every tile request (bn x stages x waves x
    channels x ksize x korder x LayerNorm fold) at M = 1 .. 257 pixels with the plain epilogue, and every epilogue (activation, time
    embedding, residual, wide stream, split-K, GroupNorm hand-over, fold) on every tile at three sample sizes and two output widths.
    Every descriptor is also given to es_conv_gemm on the dry recorder: both accept it, or both refuse it with the same text.  Between
    them the grids and _GEMM_REFUSED reach every row of the instantiation table (33 + 6 per dtype, each under one kernel id) and
    produce every refusal text gemm_check has."""
    from tests import numerics as nm
    assert lib.GEMM_ROUTE_FIELDS == nm.GEMM_ROUTE_KEYS
    rows, n = {}, 0
    with _DryPlan() as dry:
        sweep = _RouteSweep(dry, dry.L.es_conv_gemm_route, dry.L.es_conv_gemm, lib.GEMM_ROUTE_FIELDS)

        def point(d):
            got = sweep.ask(d)
            if got is not None:
                want = nm.gemm_route(d)
                assert {k: v for k, v in got.items() if k != "row"} == {k: v for k, v in want.items() if k != "row"}, (got, want)
                assert rows.setdefault(got["row"], got["kernel"] & ~0x100000) == got["kernel"] & ~0x100000
                f = lib.gemm_kernel_fields(got["kernel"])
                assert (f["bn"], f["stages"], f["waves"], f["bm"] == 256) == (got["bn"], got["stages"], got["waves"], got["family"] == 1)
            return got
        for bn in (64, 128, 160, 256, 320):
            for stages in (0, 2, 3, 4):
                for waves in (0, 4, 8):
                    for C1, C2 in ((64, 0), (128, 64), (72, 0)):
                        for ksize, korder, ln in ((1, 0, 0), (1, 0, 1), (1, 1, 0), (3, 0, 0), (3, 1, 0), (3, 1, 1)):
                            for M in (1, 64, 128, 129, 256, 257):
                                n += 1
                                point(_gemm_desc(M, C1=C1, C2=C2, ksize=ksize, bn=bn, stages=stages, waves=waves, korder=korder, ln_colsum=ln,
                                                 dtype=n & 1))
            for act in (lib.ACT_NONE, lib.ACT_SILU, lib.ACT_GEGLU):
                for temb, residual, out_lo in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 1, 1), (1, 1, 1), (0, 0, 1)):
                    for splitk in (1, 2):
                        for gn_part in (0, 1):
                            for ln in (0, 1):
                                for M, hw in ((128, 128), (256, 64), (257, 257)):
                                    for Cout in (1280, 1276):
                                        n += 1
                                        point(_gemm_desc(M, hw, C1=128, Cout=Cout, bn=bn, act=act, temb=temb, residual=residual, out_lo=out_lo,
                                                         residual_lo=out_lo and temb, splitk=splitk, workspace=1, gn_part=gn_part, ln_colsum=ln,
                                                         dtype=n & 1))
        for limit, kw in _GEMM_REFUSED:
            prev = dry.L.es_set_operand_limit(limit)
            try:
                assert point(_gemm_desc(**kw)) is None, kw
            finally:
                dry.L.es_set_operand_limit(prev)
    assert sorted(rows) == list(range(lib.GEMM_ROWS_128 + lib.GEMM_ROWS_256)) and len(set(rows.values())) == len(rows), sorted(rows)
    assert all((lib.gemm_kernel_fields(k)["bm"] == 256) == (r >= lib.GEMM_ROWS_128) for r, k in rows.items())
    missing = _source_texts("gemm_conv.hip", "es_conv_gemm") - sweep.texts
    assert not missing and len(sweep.texts) >= 35, missing


def test_conv_gemm_tile_downgrades():
    """What a descriptor recorded with the big tile runs on when the phase-interleaved kernel lacks its epilogue, as literals: bn = 320
    with SiLU, with a time embedding over samples that are no multiple of 128 pixels, with a time embedding and a residual, or with
    Cout % 8 != 0 runs the 128 x 160 tile on a ring of 2; the same four with split-K stay on the 256-pixel kernel (it writes raw partials).
    bn = 256 with SiLU, Cout % 8 != 0 or GEGLU + residual runs 128 x 128; the plain, folded and GEGLU forms stay."""
    fam = lambda **kw: tuple(lib.gemm_route(_gemm_desc(256, C1=128, **kw))[k] for k in ("family", "bn", "stages", "waves", "threads"))
    big320, big256, t160, t128 = (1, 320, 2, 8, 512), (1, 256, 2, 8, 512), (0, 160, 2, 4, 256), (0, 128, 2, 4, 256)
    for kw in (dict(act=lib.ACT_SILU), dict(temb=1, hw=64), dict(temb=1, residual=1, hw=128), dict(Cout=1276)):
        assert fam(bn=320, **kw) == t160, kw
        assert fam(bn=320, splitk=2, workspace=1, **kw) == big320, kw
    assert fam(bn=320) == fam(bn=320, temb=1, hw=128) == fam(bn=320, residual=1) == fam(bn=320, residual=1, out_lo=1) == big320
    for kw in (dict(act=lib.ACT_SILU), dict(Cout=1276), dict(act=lib.ACT_GEGLU, residual=1)):
        assert fam(bn=256, **kw) == t128, kw
    for kw in (dict(), dict(ln_colsum=1), dict(act=lib.ACT_GEGLU), dict(act=lib.ACT_GEGLU, ln_colsum=1), dict(residual=1), dict(splitk=2, workspace=1)):
        assert fam(bn=256, **kw) == big256, kw
    r = lib.gemm_route(_gemm_desc(256, C1=128, bn=320, act=lib.ACT_SILU, korder=1, ksize=3))
    assert lib.gemm_kernel_fields(r["kernel"]) == dict(bn=160, bm=128, stages=2, waves=4, aligned=True, ln=False, ko=True, geglu=False, bf16=False)
    with pytest.raises(lib.EdgeStyleHipError, match="es_conv_gemm: bn=320 is the 256-pixel phase-interleaved tile"):
        lib.gemm_route(_gemm_desc(256, C1=128, bn=320, stages=4))


def test_conv_gemm_route_counts_the_runs_of_an_oversize_launch():
    """With the operand limit lowered (es_set_operand_limit), the route's run count, samples per run and first-run grid against the
    mirror: a plain launch, a grouped one (runs never span a weight group), one whose source repeats every x_nmod samples (runs of whole
    periods), a split-K one (the reduce grid is the first run's), and a linear layer (hw = 1: cuts between 256-row tiles)."""
    from tests import numerics as nm
    L = lib.load()
    cases = [(1 << 20, dict(M=1024, hw=128), (3, 3)), (1 << 20, dict(M=2048, hw=256, groups=[6, 16]), (8, 1)),
             (1 << 22, dict(M=2560, hw=256, groups=[6, 20]), (3, 6)), (1 << 22, dict(M=2560, hw=256, x_nmod=2), (2, 6)),
             (1 << 20, dict(M=1024, hw=128, splitk=2, C1=128, workspace=1), (3, 3)), (1 << 22, dict(M=4096, hw=1), (3, 1536))]           # 2560 B per row: 1638 rows fit, 1536 in whole 256-row tiles
    for limit, kw, (runs, per) in cases:
        prev = L.es_set_operand_limit(limit)
        try:
            d = _gemm_desc(**kw)
            got, want = lib.gemm_route(d), nm.gemm_route(d, limit)
        finally:
            L.es_set_operand_limit(prev)
        assert {k: v for k, v in got.items() if k != "row"} == {k: v for k, v in want.items() if k != "row"}, (kw, got, want)
        assert (got["runs"], got["samples_per_run"]) == (runs, per), (kw, got)
        assert lib.gemm_route(d)["runs"] == 1


def test_conv_gemm_production_routes():
    """Which kernel the launches of a 512 x 512 batch-1 step go to: what es_launch_choose picks at default knobs for the layers
    test_every_knob_bends_the_launch_choice_as_before enumerates (those it sends to es_conv_gemm), laid into a descriptor and routed.
    DESIGN section 4: the 3x3 convolutions of the grouped encoder's 64 x 64 level and the GEGLU of that level run the 256-pixel
    phase-interleaved kernel, short-K 1x1 layers the 128-pixel tile on 8 waves, tiny launches the 64 x 64 tile (a ring of 4 where K is
    long), split-K launches the 4-wave tile with the plain reduce.  The literals are a first run's; none contradicts DESIGN."""
    L = lib.load()

    def route(cin, cout, k, M, hw, geglu=False, **facts):
        bn = 128 if geglu else ops.choose_bn(cout)
        pw = ops.PackedWeight(torch.empty(-(-cout // bn) * bn, k * k * cin, device="meta"), None, cout, cin, k, bn, geglu,
                              ln_colsum=torch.empty(0) if geglu else None)
        ch, q = lib.LaunchChoice(), ops.launch_query(M, hw, pw, C1=cin, src_numel=M * cin, **facts)
        assert L.es_launch_choose(ctypes.byref(q), ctypes.byref(ops.launch_knobs()), ctypes.byref(ch)) == 0 and ch.route == lib.ROUTE_CONV_GEMM
        r = lib.gemm_route(_gemm_desc(M, hw, C1=cin, ksize=k, Cout=cout, bn=ch.bn, splitk=ch.splitk, stages=ch.stages, waves=ch.waves,
                                      workspace=1, act=lib.ACT_GEGLU if geglu else 0, ln_colsum=geglu))
        return r["family"], r["bn"], r["stages"], r["waves"], r["reduce"]
    assert route(320, 960, 1, 1024, 1024) == (0, 64, 2, 4, 0)
    assert route(320, 320, 1, 256, 256) == (0, 64, 2, 4, 0)
    assert route(1280, 1280, 1, 4096, 4096) == (0, 128, 2, 8, 0)
    assert route(320, 320, 3, 57344, 4096) == (1, 320, 2, 8, 0)
    assert route(320, 640, 3, 57344, 4096) == (1, 320, 2, 8, 0)
    assert route(1280, 1280, 1, 1024, 1024) == (0, 64, 4, 4, 0)
    assert route(320, 320, 3, 8192, 4096, gn_groups=32) == (0, 160, 2, 4, lib.GEMM_REDUCE_PLAIN)
    assert route(1280, 1280, 3, 512, 256, gn_groups=32) == (0, 128, 2, 4, lib.GEMM_REDUCE_PLAIN)
    assert route(1280, 10240, 1, 28672, 4096, geglu=True) == (1, 256, 2, 8, 0)


def test_conv_gemm_last_kernel_is_set_by_launches_only():
    """es_conv_gemm_last_kernel: written by the launchers alone - 0 in a process that has launched nothing (no GPU: this one), and a dry
    recording call or a route query leaves it as it was; the bit layout is the header's"""
    L = lib.load()
    before = L.es_conv_gemm_last_kernel()
    if not torch.cuda.is_available():
        assert before == 0
    with _DryPlan() as dry:
        assert L.es_conv_gemm(ctypes.byref(_gemm_desc()), None) == 0 and dry.size() == 1
        assert lib.gemm_route(_gemm_desc())["kernel"] != 0 and L.es_conv_gemm_last_kernel() == before
    hdr = open(os.path.join(ROOT, "include", "edgestyle_hip.h")).read()
    bits = {name: int(v, 0) for name, v in re.findall(r"ES_GEMM_KERNEL_(\w+) = (0x[0-9A-Fa-f]+|\d+)", hdr)}
    all_on = bits["BN_MASK"] | bits["BM64_MASK"] << bits["BM64_SHIFT"] | bits["STAGES_MASK"] << bits["STAGES_SHIFT"] | bits["WAVES8"] | \
        bits["ALIGNED"] | bits["LN"] | bits["KO"] | bits["GEGLU"] | bits["BF16"]
    assert lib.gemm_kernel_fields(all_on) == dict(bn=0x1FF, bm=64 * 7, stages=7, waves=8, aligned=True, ln=True, ko=True, geglu=True, bf16=True)
    assert all_on == (1 << 21) - 1


# one descriptor per refusal of xs_check that the sweep below does not meet
_XS_REFUSED = [
    (0, dict(K=384)), (0, dict(Cout=96)), (0, dict(chunks_per_slice=4)), (0, dict(ldo=324)), (0, dict(rows_padded=1 << 22)), (0, dict(ngroups=5)),
    (0, dict(gn_part=1, gn_gamma=1, gn_beta=1, residual=1)), (0, dict(gn_part=1, gn_gamma=1, gn_beta=1, gn_hw=300)), (0, dict(gn_part=1)),
    (0, dict(gn_part=1, groups=[2, 4], gn_gamma_g=(ctypes.c_void_p * 4)())), (0, dict(M=1024, gn_part=1, gn_hw=512, groups=[2, 8])),
    (0, dict(residual=1, K=640)), (0, dict(groups=[3, 4])), (0, dict(groups=[2, 5])),
    (1 << 19, dict(M=2048, Cout=320, gn_part=1, gn_gamma=1, gn_beta=1, gn_hw=1024)),
]


def test_linear_xs_route_is_the_mirrors_answer_and_refuses_what_the_launch_refuses():
    """es_linear_xs_route (xs_route of csrc/linear_xs.hip, which es_linear_xs launches from) against the Python restatement (tests/numerics.py
    xs_route) over K x GEGLU x LayerNorm x residual x GroupNorm-in-front x ping-pong knob x M x slices, and - operand limit lowered - over
    launches cut into runs, grouped and with GroupNorm in front.  Every descriptor also goes to es_linear_xs on the dry recorder: both
    accept, or both refuse with the same text.  The grid reaches all 16 instantiations, the grid and _XS_REFUSED every text of xs_check."""
    from tests import numerics as nm
    assert lib.XS_ROUTE_FIELDS == nm.XS_ROUTE_KEYS
    forms = set()
    with _DryPlan() as dry:
        sweep = _RouteSweep(dry, dry.L.es_linear_xs_route, dry.L.es_linear_xs, lib.XS_ROUTE_FIELDS, knobs=True)
        for K in (320, 640):
            for geglu, ln, residual, gn in ((0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 1, 0), (0, 1, 1, 0),
                                            (1, 0, 0, 1), (0, 1, 0, 1)):
                for pp in (0, 1):
                    for M in (1, 255, 256, 257, 513):
                        for nslices in (1, 2, 3):
                            d = _xs_desc(M, K, nslices=nslices, geglu=geglu, ln=ln, residual=residual, gn_part=gn, gn_gamma=gn, gn_beta=gn, dtype=M & 1)
                            got = sweep.ask(d, ctypes.byref(lib.XsKnobs(pp)))
                            if got is not None:
                                assert got == nm.xs_route(d, pp), (got, nm.xs_route(d, pp))
                                forms.add(got["form"])
        assert forms == {nm.xs_form_id(*f) for f in nm.XS_FORMS} and len(forms) == 16
        # (1 MiB over rows of 1280 B: 819 rows less one block of slack, 512 in whole blocks; 3 + 6 runs of the groups of 1536 and 2561 rows;
        #  a limit below two blocks, or rows of 2560 B: single blocks)
        for limit, kw, (runs, rows) in [(1 << 20, dict(M=4096), (8, 512)), (1 << 20, dict(M=4097, groups=[12, 33]), (9, 512)),
                                        (1 << 20, dict(M=4096, gn_part=1, gn_gamma=1, gn_beta=1, gn_hw=512), (8, 512)),
                                        (1 << 16, dict(M=700), (3, 256)), (1 << 20, dict(M=4096, K=640, geglu=1, Cout=2560), (16, 256))]:
            prev = dry.L.es_set_operand_limit(limit)
            try:
                d = _xs_desc(**kw)
                got = sweep.ask(d, None)
                assert got == nm.xs_route(d, 1, limit) and (got["runs"], got["rows_per_run"]) == (runs, rows), (kw, got, nm.xs_route(d, 1, limit))
            finally:
                dry.L.es_set_operand_limit(prev)
        for limit, kw in _XS_REFUSED:
            prev = dry.L.es_set_operand_limit(limit)
            try:
                assert sweep.ask(_xs_desc(**kw), None) is None, kw
            finally:
                dry.L.es_set_operand_limit(prev)
    missing = _source_texts("linear_xs.hip", "es_linear_xs") - sweep.texts
    assert not missing and len(sweep.texts) >= 15, missing


def test_linear_xs_knobs_are_read_on_first_use_and_follow_set_pp():
    """ES_XS_PP is read on first use, not when the library is loaded: a child process that sets it to 0 AFTER loading the library gets
    the one-barrier form from its first route query; unset, the default is the ping-pong form; es_linear_xs_set_pp edits the struct
    es_linear_xs_knobs copies and the route follows it"""
    import subprocess
    import sys
    from tests import numerics as nm
    child = ("import os, sys; sys.path.insert(0, %r); from edgestyle_amd import lib; L = lib.load(); os.environ['ES_XS_PP'] = '0'; "
             "d, k = lib.XsDesc(), lib.XsKnobs(); d.M, d.K, d.Cout, d.rows_padded, d.ldo, d.nslices, d.chunks_per_slice = 512, 320, 640, 640, 640, 1, 10; "
             "r = lib.xs_route(d); L.es_linear_xs_knobs(k); print(r['form'], k.pp)" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "ES_XS_PP"}
    out = subprocess.run([sys.executable, "-c", child], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [nm.xs_form_id(320, "plain", 0), 0], out
    if "ES_XS_PP" in os.environ:
        return
    L, k = lib.load(), lib.XsKnobs()
    L.es_linear_xs_knobs(k)
    first = k.pp
    assert L.es_linear_xs_set_pp(0) == first
    try:
        L.es_linear_xs_knobs(k)
        assert k.pp == 0 and lib.xs_route(_xs_desc())["form"] == nm.xs_form_id(320, "plain", 0)
        assert lib.xs_route(_xs_desc(), lib.XsKnobs(1))["form"] == nm.xs_form_id(320, "plain", 1)
        assert lib.xs_route(_xs_desc(gn_part=1, gn_gamma=1, gn_beta=1))["form"] == nm.xs_form_id(320, "gn", 1)
        assert L.es_linear_xs_set_pp(1) == 0 and lib.xs_route(_xs_desc())["form"] == nm.xs_form_id(320, "plain", 1)
    finally:
        L.es_linear_xs_set_pp(first)
    L.es_linear_xs_knobs(k)
    assert k.pp == first == 1
