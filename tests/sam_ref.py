"""The EfficientViT-SAM image encoder (EfficientViTLargeBackbone + SamNeck + LayerNorm2d) restated in plain torch functions over a
state dict that carries the reference's own key names.  One walk of the network (`Net.forward`) serves four purposes:

  mode "fp64"     the truth the kernels are judged against;
  mode "fp32"     what the reference computes without autocast (the host baseline of tools/sam_encoder_bench.py);
  mode "rounded"  the textbook op sequence in fp32 with every op's output (convolution, BatchNorm, GELU, add, upsample, attention,
                  LayerNorm) and every convolution weight rounded to the storage dtype: the `base_ref` of tests/NUMERICS.md;
  gen = seed      the same walk creates the tensors it does not find (`random_state_dict`): seeded weights and biases, BatchNorm
                  weight / bias / running_mean / running_var all randomised (the defaults would make the fold trivial), and every
                  convolution scaled by a POWER OF TWO so that its output has a standard deviation near 1 on a seeded probe image.
                  Powers of two keep the state dict bit-for-bit reproducible: a different summation order in the probe pass moves
                  a measured deviation by 1e-7, never across a rounding boundary of log2.  `Net.stats` records the standard
                  deviation of every layer's output; `assert_stats` is the postcondition (all in [0.1, 10]).

Whether a ConvLayer has a bias or a BatchNorm is read from the keys that exist, as the library does.
`sam_resize_shape` restates SamResize.get_preprocess_shape; `preprocess_ref` the whole EfficientViTSam.transform on Pillow.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

L_WIDTHS = (32, 64, 128, 256, 512)
MODELS = {"l0": ((1, 1, 1, 4, 4), 4), "l1": ((1, 1, 1, 6, 6), 8), "l2": ((1, 2, 2, 8, 8), 12)}
PIXEL_MEAN = (123.675 / 255, 116.28 / 255, 103.53 / 255)
PIXEL_STD = (58.395 / 255, 57.12 / 255, 57.375 / 255)
NECK_SIZE = 64
ATT_EPS = 1.0e-15
BRANCH = 0.25          # a power of two, like every scale of the generator


def config(widths=L_WIDTHS, depths=(1, 2, 2, 8, 8), head_width=256, head_depth=12, out_dim=256, image_size=512, qkv_dim=32,
           bn_eps=1e-6, ln_eps=1e-6):
    return dict(widths=tuple(widths), depths=tuple(depths), head_width=head_width, head_depth=head_depth, out_dim=out_dim,
                image_size=image_size, qkv_dim=qkv_dim, bn_eps=bn_eps, ln_eps=ln_eps)


def model_config(name, image_size=512):
    depths, head_depth = MODELS[name]
    return config(depths=depths, head_depth=head_depth, image_size=image_size)


# the fixture's network (tests/golden/make_golden_ref_sam.py): the smallest widths the library runs; out_dim 8 keeps the stored
# [1, out_dim, 64, 64] fp64 outputs of two inputs under the size limit of a committed file
TINY = config(widths=(32, 32, 64, 64, 64), depths=(1, 1, 1, 1, 1), head_width=64, head_depth=1, out_dim=8, image_size=64)
TINY_SEED = 20240
# real widths, one block per stage: every channel count of the real model, the 6144-channel depthwise launch included
SHALLOW = config(depths=(1, 1, 1, 1, 1), head_depth=1, image_size=128)


def rnd(x, dtype):
    return x.to(torch.float32).to(dtype).to(torch.float32)


def gelu_tanh(x):
    return F.gelu(x, approximate="tanh")


def relu_linear_att(ms, dim=32, eps=ATT_EPS):
    """LiteMLA.relu_linear_att: ms [B, groups * 3 * dim, H, W] -> [B, groups * dim, H, W]"""
    B, _, H, W = ms.shape
    t = ms.reshape(B, -1, 3 * dim, H * W).transpose(-1, -2)
    q, k, v = torch.relu(t[..., :dim]), torch.relu(t[..., dim:2 * dim]), t[..., 2 * dim:]
    v = F.pad(v, (0, 1), mode="constant", value=1)
    out = torch.matmul(q, torch.matmul(k.transpose(-1, -2), v))
    out = out[..., :-1] / (out[..., -1:] + eps)
    return out.transpose(-1, -2).reshape(B, -1, H, W)


class Net:
    def __init__(self, cfg, sd=None, mode="fp64", dtype=None, gen=None):
        assert mode in ("fp64", "fp32", "rounded") and (mode != "rounded" or dtype is not None)
        self.cfg, self.mode, self.dtype = cfg, mode, dtype
        self.sd = {} if sd is None else sd
        self.gen = gen
        self.ct = torch.float64 if mode == "fp64" else torch.float32
        self.stats = {}

    # ---- leaves ----
    def r(self, t):
        return rnd(t, self.dtype) if self.mode == "rounded" else t

    def p(self, key, weight=False):
        t = self.sd[key].to(self.ct)
        return rnd(t, self.dtype) if (weight and self.mode == "rounded") else t

    def _randn(self, *shape):
        return torch.randn(*shape, generator=self.gen, dtype=torch.float32)

    def _rand(self, lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(*shape, generator=self.gen, dtype=torch.float32)

    def conv(self, p, x, cin, cout, k, stride=1, groups=1, bias=False, norm=True, act=False, raw=False, gain=1.0):
        """ConvLayer `p` (conv [+ BatchNorm] [+ tanh-GELU]); raw: a bare nn.Conv2d whose keys are p.weight / p.bias; gain: the deviation the
        generator scales the convolution's output to (BRANCH for the last convolution of a residual branch: the stream of the deepest
        model, 17 adds in stage4, then stays inside the postcondition)"""
        wk = p + (".weight" if raw else ".conv.weight")
        bk = p + (".bias" if raw else ".conv.bias")
        if self.gen is not None and wk not in self.sd:
            fan = (cin // groups) * k * k
            w = self._randn(cout, cin // groups, k, k) / math.sqrt(fan)
            y = F.conv2d(x, w.to(self.ct), None, stride, k // 2, 1, groups)
            scale = gain * 2.0 ** round(math.log2(1.0 / max(float(y.float().std()), 1e-30)))
            self.sd[wk] = w * scale
            if bias:
                self.sd[bk] = 0.1 * self._randn(cout)
            if norm:
                self.sd[p + ".norm.weight"] = self._rand(0.5, 1.5, cout)
                self.sd[p + ".norm.bias"] = 0.2 * self._randn(cout)
                self.sd[p + ".norm.running_mean"] = 0.2 * self._randn(cout)
                self.sd[p + ".norm.running_var"] = self._rand(0.5, 1.5, cout)
        w = self.p(wk, weight=True)
        assert tuple(w.shape) == (cout, cin // groups, k, k), (wk, tuple(w.shape))
        b = self.p(bk) if bk in self.sd else None
        y = self.r(F.conv2d(x, w, b, stride, k // 2, 1, groups))
        if not raw and p + ".norm.weight" in self.sd:
            g, bt = self.p(p + ".norm.weight"), self.p(p + ".norm.bias")
            m, v = self.p(p + ".norm.running_mean"), self.p(p + ".norm.running_var")
            y = (y - m.view(1, -1, 1, 1)) / torch.sqrt(v.view(1, -1, 1, 1) + self.cfg["bn_eps"]) * g.view(1, -1, 1, 1) + bt.view(1, -1, 1, 1)
            y = self.r(y)
        if act:
            y = self.r(gelu_tanh(y))
        self.stats[p] = float(y.float().std())
        return y

    def add(self, name, a, b):
        y = self.r(a + b)
        self.stats[name] = float(y.float().std())
        return y

    # ---- blocks ----
    def res_block(self, p, x, c):
        y = self.conv(p + ".main.conv1", x, c, c, 3, act=True)
        y = self.conv(p + ".main.conv2", y, c, c, 3, gain=BRANCH)
        return self.add(p, y, x)

    def fmb(self, p, x, cin, cout, stride, expand, shortcut):
        mid = round(cin * expand)
        y = self.conv(p + ".main.spatial_conv", x, cin, mid, 3, stride, act=True)
        y = self.conv(p + ".main.point_conv", y, mid, cout, 1, gain=BRANCH if shortcut else 1.0)
        return self.add(p, y, x) if shortcut else y

    def mb(self, p, x, cin, cout, stride, expand, shortcut, fewer_norm=True):
        mid = round(cin * expand)
        y = self.conv(p + ".main.inverted_conv", x, cin, mid, 1, bias=fewer_norm, norm=not fewer_norm, act=True)
        y = self.conv(p + ".main.depth_conv", y, mid, mid, 3, stride, groups=mid, bias=fewer_norm, norm=not fewer_norm, act=True)
        y = self.conv(p + ".main.point_conv", y, mid, cout, 1, gain=BRANCH if shortcut else 1.0)
        return self.add(p, y, x) if shortcut else y

    def lite_mla(self, p, x, c):
        dim = self.cfg["qkv_dim"]
        heads = c // dim
        qkv = self.conv(p + ".main.qkv", x, c, 3 * c, 1, norm=False)
        agg = self.conv(p + ".main.aggreg.0.0", qkv, 3 * c, 3 * c, 5, groups=3 * c, norm=False, raw=True)
        agg = self.conv(p + ".main.aggreg.0.1", agg, 3 * c, 3 * c, 1, groups=3 * heads, norm=False, raw=True)
        ms = torch.cat([qkv, agg], dim=1)
        att = relu_linear_att(ms if self.mode == "fp64" else ms.float(), dim).to(self.ct)      # @autocast(enabled=False): fp32
        att = self.r(att)
        self.stats[p + ".main.att"] = float(att.float().std())
        y = self.conv(p + ".main.proj", att, 2 * c, c, 1, gain=BRANCH)
        return self.add(p, y, x)

    # ---- the network ----
    def forward(self, x):
        """x [B, 3, S, S] -> dict(stage2, stage3, stage4, out [B, out_dim, 64, 64])"""
        cfg = self.cfg
        w, d = cfg["widths"], cfg["depths"]
        x = self.r(x.to(self.ct))
        p = "backbone.stages.0.op_list."
        x = self.conv(p + "0", x, 3, w[0], 3, 2, act=True)
        for i in range(d[0]):
            x = self.res_block(p + str(1 + i), x, w[0])
        feats = {}
        cin = w[0]
        for s in (1, 2, 3):
            p = f"backbone.stages.{s}.op_list."
            for i in range(d[s] + 1):
                stride, expand = (2, 16) if i == 0 else (1, 4)
                if s <= 2:
                    x = self.fmb(p + str(i), x, cin, w[s], stride, expand, stride == 1)
                else:
                    x = self.mb(p + str(i), x, cin, w[s], stride, expand, stride == 1)
                cin = w[s]
            feats[f"stage{s}"] = x
        p = "backbone.stages.4.op_list."
        x = self.mb(p + "0", x, cin, w[4], 2, 24, False)
        for i in range(d[4]):
            x = self.lite_mla(p + f"{1 + i}.context_module", x, w[4])
            x = self.mb(p + f"{1 + i}.local_module", x, w[4], w[4], 1, 6, True)
        feats["stage4"] = x
        hw = cfg["head_width"]
        ups = []
        for j, s in enumerate((4, 3, 2)):
            y = self.conv(f"neck.input_ops.{j}.op_list.0", feats[f"stage{s}"], w[s], hw, 1)
            if tuple(y.shape[-2:]) != (NECK_SIZE, NECK_SIZE):
                y = self.r(F.interpolate(y, size=(NECK_SIZE, NECK_SIZE), mode="bicubic", align_corners=False))
            ups.append(y)
        y = self.r(ups[0] + self.r(ups[1] + ups[2]))          # list_sum: x[0] + list_sum(x[1:])
        self.stats["neck.merge"] = float(y.float().std())
        for i in range(cfg["head_depth"]):
            y = self.fmb(f"neck.middle.op_list.{i}", y, hw, hw, 1, 1, True)
        y = self.conv("neck.output_ops.0.op_list.0", y, hw, cfg["out_dim"], 1, bias=True, norm=False)
        if self.gen is not None and "norm.weight" not in self.sd:
            self.sd["norm.weight"] = self._rand(0.5, 1.5, cfg["out_dim"])
            self.sd["norm.bias"] = 0.2 * self._randn(cfg["out_dim"])
        o = y - y.mean(dim=1, keepdim=True)
        o = o / torch.sqrt(o.square().mean(dim=1, keepdim=True) + cfg["ln_eps"])
        o = self.r(o * self.p("norm.weight").view(1, -1, 1, 1) + self.p("norm.bias").view(1, -1, 1, 1))
        self.stats["norm"] = float(o.float().std())
        feats["out"] = o
        return feats


def probe_image(size, n=1, seed=7, dtype=torch.bfloat16):
    """a seeded image-like input [n, 3, size, size], exact in fp16 and in bf16"""
    g = torch.Generator().manual_seed(seed)
    return rnd(torch.randn(n, 3, size, size, generator=g) * 1.2, dtype)


def random_state_dict(cfg, seed=0, probe_size=128):
    """state dict under the reference's key names for `cfg` (see the module docstring)"""
    g = torch.Generator().manual_seed(seed)
    net = Net(cfg, None, "fp32", gen=g)
    with torch.no_grad():
        net.forward(probe_image(probe_size, seed=seed + 1))
    return {k: v.contiguous() for k, v in net.sd.items()}


def assert_stats(stats, lo=0.1, hi=10.0):
    bad = {k: v for k, v in stats.items() if not (lo <= v <= hi)}
    assert not bad, f"layer outputs with a standard deviation outside [{lo}, {hi}]: {bad}"


def forward(cfg, sd, x, mode="fp64", dtype=None, want_stats=False):
    net = Net(cfg, sd, mode, dtype)
    with torch.no_grad():
        out = net.forward(x)
    return (out, net.stats) if want_stats else out


def state_dict_sums(sd):
    """per-tensor (sum, sum of squares) in fp64, keys sorted: what the fixture stores to notice a generator that drifted"""
    keys = sorted(sd)
    return keys, torch.tensor([[float(sd[k].double().sum()), float(sd[k].double().square().sum())] for k in keys], dtype=torch.float64)


class RefModule(torch.nn.Module):
    """an nn.Module with the reference's parameter and buffer names whose forward is the fp32 restatement: what
    NativeSamImageEncoder.from_module takes in place of EfficientViTSamImageEncoder"""

    def __init__(self, cfg, sd):
        super().__init__()
        self.cfg = cfg
        self._names = {}
        for k, v in sd.items():
            flat = k.replace(".", "__")
            self._names[flat] = k
            if "running_" in k:
                self.register_buffer(flat, v.clone())
            else:
                self.register_parameter(flat, torch.nn.Parameter(v.clone(), requires_grad=False))

    def state_dict(self, *a, **kw):
        return {self._names[k]: v for k, v in super().state_dict(*a, **kw).items()}

    def forward(self, x):
        return forward(self.cfg, self.state_dict(), x, "fp32")["out"]


# ---- preprocessing -------------------------------------------------------------------------------------------------------------
def sam_resize_shape(oldh, oldw, long_side):
    scale = long_side * 1.0 / max(oldh, oldw)
    newh, neww = oldh * scale, oldw * scale
    return int(newh + 0.5), int(neww + 0.5)


def preprocess_ref(img_u8, S):
    """EfficientViTSam.transform on an HxWx3 uint8 array: (resized bytes [h, w, 3], fp32 [3, S, S], (h, w))"""
    from PIL import Image
    h, w = img_u8.shape[:2]
    nh, nw = (h, w) if max(h, w) == S else sam_resize_shape(h, w, S)
    pil = Image.fromarray(np.ascontiguousarray(img_u8[..., :3]))
    if (nh, nw) != (h, w):
        pil = pil.resize((nw, nh), Image.BILINEAR)
    b = np.asarray(pil)
    t = torch.from_numpy(b.copy()).permute(2, 0, 1).to(torch.float32).div(255)
    mean = torch.tensor(PIXEL_MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(PIXEL_STD, dtype=torch.float32).view(3, 1, 1)
    t = (t - mean) / std
    out = torch.zeros(3, S, S, dtype=torch.float32)
    out[:, :nh, :nw] = t
    return b, out, (nh, nw)
