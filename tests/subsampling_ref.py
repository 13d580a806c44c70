"""Float64 references for Conv2dSubsampling (espnet/nets/pytorch_backend/transformer/
subsampling.py:46-91) and its HIP kernels; no GPU code.

* `subsampling_f64`: the whole layer, forward + backward, optionally rounding to bf16 where the
  implicit-GEMM path stores bf16, with an optional dropout mask and absolute-PE table.
* `phase_split` / `phase_unsplit` (and `pos_split` / `pos_unsplit` for the ReLU support bits):
  NHWC (B, T1, F1, C) <-> the x1p row order of ea_conv_geo / layers.subsampling.phase_geo.
* per-mode references written as index restatements (strided slices, no conv2d): conv2
  forward, input gradient (conv1 ReLU mask from x1 > 0), weight gradient in (Co, 9, Ci) order;
  conv1 forward, weight and bias gradients.
* the integer grid: inputs from small integer sets, so that every product and every partial sum
  of every result is an integer of magnitude < 2**24.  f32 accumulation is then exact in any
  order and under any split of the sum, a kernel's result is determined to the bit (the only
  rounding left is a final bf16 store, which `.to(torch.bfloat16)` reproduces), and the
  comparison is `torch.equal`.  `assert_f32_exact` checks the condition on the reference
  evaluated on the inputs' magnitudes: that bounds every partial sum in every order.
"""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64


def bf(x):
    """Round to bf16 (round-to-nearest-even), keep float64."""
    return x.to(torch.bfloat16).to(F64)


# ------------------------------------------------------------------------------ the layer
def subsampling_f64(P, feats, gy, emulate_bf16, mask=None, pe=None, dt=F64, route="implicit"):
    """Conv2dSubsampling fwd + bwd.  emulate_bf16: round where the implicit-GEMM path stores
    bf16; with route="im2col", where the im2col route does: that route also feeds conv1's GEMM
    the bf16 input and weight, and stores every tap's share of conv2's input gradient in bf16
    (the dcol buffer) before col2im sums them.  mask (B, T2, C): the dropout keep mask already
    divided by (1 - p), applied to the output (and to gy in the backward); pe (>= T2, C): absolute PositionalEncoding rows added
    before the mask (embedding.py:81-92).  dt: the arithmetic (float64; float32 measures the
    f32 floor of the same restatement).  Returns (y, {param: grad})."""
    r = (lambda t: t.to(torch.bfloat16).to(dt)) if emulate_bf16 else (lambda t: t)
    P = {k: v.to(dt) for k, v in P.items()}
    feats, gy = feats.to(dt), gy.to(dt)
    W1, b1 = P["conv.0.weight"], P["conv.0.bias"]
    W2, b2 = P["conv.2.weight"], P["conv.2.bias"]
    Wl, bl = P["out.0.weight"], P["out.0.bias"]
    C = W1.shape[0]
    xs = math.sqrt(C)
    x = feats.unsqueeze(1)
    im2col = emulate_bf16 and route == "im2col"
    if im2col:
        x, W1 = r(x), r(W1)
    x1 = r(torch.relu(F.conv2d(x, W1, b1, stride=2)))              # (B, C, T1, F1)
    W2r = r(W2)
    x2 = r(torch.relu(F.conv2d(x1, W2r, b2, stride=2)))            # (B, C, T2, F2)
    B, _, T2, F2 = x2.shape
    xr = x2.transpose(1, 2).reshape(B, T2, C * F2)                   # subsampling.py:66-69
    Wlr = r(Wl)
    y = (xr @ Wlr.t() + bl) * xs
    if pe is not None:
        y = y + pe[:T2].to(dt)
    if mask is not None:
        y = y * mask.to(dt)
        gy = gy * mask.to(dt)
    g = {}
    gs = gy * xs
    dv = r(gs)
    g["out.0.bias"] = dv.reshape(-1, C).sum(0)  # the column sums of the (bf16) dv
    g["out.0.weight"] = dv.reshape(-1, C).t() @ xr.reshape(-1, C * F2)
    dxr = (dv @ Wlr).reshape(B, T2, C, F2).transpose(1, 2)           # (B, C, T2, F2)
    dh2 = r(dxr * (x2 > 0))
    g["conv.2.bias"] = dh2.sum((0, 2, 3))
    g["conv.2.weight"] = torch.nn.grad.conv2d_weight(x1, W2.shape, dh2, stride=2)
    if im2col:
        d1 = torch.zeros_like(x1).permute(0, 2, 3, 1)                # NHWC view
        dn, w9 = dh2.permute(0, 2, 3, 1), W2r.reshape(C, C, 9)
        for q, v in enumerate(_taps(d1, T2, F2)):
            v += r(dn @ w9[:, :, q])
        dx1 = r(d1.permute(0, 3, 1, 2) * (x1 > 0))
    else:
        dx1 = r(torch.nn.grad.conv2d_input(x1.shape, W2r, dh2, stride=2) * (x1 > 0))
    g["conv.0.bias"] = dx1.sum((0, 2, 3))
    g["conv.0.weight"] = torch.nn.grad.conv2d_weight(x, W1.shape, dx1, stride=2)
    return y, g


# ------------------------------------------------------------------------------ phase split
PLANES = ((0, 0), (0, 1), (1, 0), (1, 1))


def down(n):
    """Output length of a 3-wide, stride-2 window over n."""
    return (n - 3) // 2 + 1


def plane_rows(B, T1, F1):
    """Rows of the four class planes (a, e): pixels t1 = 2i + a, f1 = 2j + e."""
    nI, nJ = ((T1 + 1) // 2, T1 // 2), ((F1 + 1) // 2, F1 // 2)
    return [B * nI[a] * nJ[e] for a, e in PLANES]


def phase_split(x1, B, T1, F1, C):
    """NHWC (B, T1, F1, C) -> x1p (B*T1*F1, C): plane (a, e) dense as [b][i][j][C], planes in
    the order (0,0), (0,1), (1,0), (1,1)."""
    x1 = x1.reshape(B, T1, F1, C)
    return torch.cat([x1[:, a::2, e::2].reshape(-1, C) for a, e in PLANES], 0)


def phase_unsplit(x1p, B, T1, F1, C):
    out = x1p.new_empty(B, T1, F1, C)
    o = 0
    for (a, e), n in zip(PLANES, plane_rows(B, T1, F1)):
        out[:, a::2, e::2] = x1p[o:o + n].reshape(B, (T1 - a + 1) // 2, (F1 - e + 1) // 2, C)
        o += n
    return out


def pack_bits(m):
    """bool (rows, C) -> uint8 (rows * C/8): byte c/8 of a row, bit c & 7."""
    rows, C = m.shape
    w = (1 << torch.arange(8, dtype=torch.int32))
    return (m.reshape(rows, C // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8).reshape(-1)


def unpack_bits(b, C):
    b = b.reshape(-1, C // 8, 1).to(torch.int32)
    return ((b >> torch.arange(8, dtype=torch.int32)) & 1).bool().reshape(-1, C)


def pos_split(m, B, T1, F1, C):
    """bool NHWC support mask -> ea_conv1_fwd2's packed pos bytes in x1p row order."""
    return pack_bits(phase_split(m, B, T1, F1, C))


def pos_unsplit(b, B, T1, F1, C):
    return phase_unsplit(unpack_bits(b, C), B, T1, F1, C)


# ------------------------------------------------------------------------------ per-mode refs
def _taps(x, n2, m2):
    """The nine stride-2 tap views of a (B, N, M, ...) grid, (kh, kw) row-major."""
    return [x[:, kh:kh + 2 * n2 - 1:2, kw:kw + 2 * m2 - 1:2] for kh in range(3) for kw in range(3)]


def conv2_fwd_ref(x1, W2):
    """x1 (B, T1, F1, Ci), W2 (Co, Ci, 3, 3) -> (B, T2, F2, Co), no bias."""
    T2, F2 = down(x1.shape[1]), down(x1.shape[2])
    w = W2.reshape(W2.shape[0], W2.shape[1], 9)
    return sum(v @ w[:, :, q].t() for q, v in enumerate(_taps(x1, T2, F2)))


def conv2_dgrad_ref(x1, W2, dY2):
    """Input gradient of conv2 times conv1's ReLU mask (x1 > 0): (B, T1, F1, Ci)."""
    T2, F2 = dY2.shape[1:3]
    w = W2.reshape(W2.shape[0], W2.shape[1], 9)
    dx1 = torch.zeros_like(x1)
    for q, v in enumerate(_taps(dx1, T2, F2)):
        v += dY2 @ w[:, :, q]
    return dx1 * (x1 > 0)


def conv2_wgrad_ref(x1, dY2):
    """Weight gradient of conv2 in the (Co, 9, Ci) order ea_gemm_conv EA_CONV_WGRAD writes."""
    T2, F2 = dY2.shape[1:3]
    Co = dY2.shape[-1]
    return torch.stack([dY2.reshape(-1, Co).t() @ v.reshape(-1, x1.shape[-1]) for v in _taps(x1, T2, F2)], 1)


def conv1_fwd_ref(x, w1, b1):
    """x (B, T, F), w1 (C, 9), b1 (C) -> relu(conv1) as (B, T1, F1, C)."""
    T1, F1 = down(x.shape[1]), down(x.shape[2])
    return torch.relu(sum(v.unsqueeze(-1) * w1[:, q] for q, v in enumerate(_taps(x, T1, F1))) + b1)


def conv1_wgrad_ref(x, g):
    """g (B, T1, F1, C) = gradient of conv1's pre-activation -> dw (C, 9), dbias (C)."""
    T1, F1 = g.shape[1:3]
    C = g.shape[-1]
    dw = torch.stack([(v.unsqueeze(-1) * g).reshape(-1, C).sum(0) for v in _taps(x, T1, F1)], 1)
    return dw, g.reshape(-1, C).sum(0)


def im2col_conv1_ref(x):
    """(B, T, F) -> (B*T1*F1, 16): 9 taps, columns 9..15 zero."""
    T1, F1 = down(x.shape[1]), down(x.shape[2])
    col = x.new_zeros(x.shape[0] * T1 * F1, 16)
    for q, v in enumerate(_taps(x, T1, F1)):
        col[:, q] = v.reshape(-1)
    return col


def im2col_conv2_ref(x1):
    """(B, T1, F1, C) -> (B*T2*F2, 9*C), column (kh, kw, c)."""
    T2, F2 = down(x1.shape[1]), down(x1.shape[2])
    C = x1.shape[-1]
    return torch.stack([v.reshape(-1, C) for v in _taps(x1, T2, F2)], 1).reshape(-1, 9 * C)


def col2im_conv2_ref(dcol, x1):
    """dcol (B*T2*F2, 9*C) scattered back onto (B, T1, F1, C), times (x1 > 0)."""
    B, T1, F1, C = x1.shape
    T2, F2 = down(T1), down(F1)
    d = dcol.reshape(B, T2, F2, 9, C)
    dx1 = torch.zeros_like(x1)
    for q, v in enumerate(_taps(dx1, T2, F2)):
        v += d[:, :, :, q]
    return dx1 * (x1 > 0)


# ------------------------------------------------------------------------------ integer grid
LIMIT = float(2 ** 24)


def int_grid(shape, values, gen, zeros=0):
    """float64 tensor with entries drawn uniformly from `values`; `zeros` extra zero slots in
    the draw make the set sparser."""
    vals = torch.tensor(list(values) + [0] * zeros, dtype=F64)
    return vals[torch.randint(len(vals), tuple(shape), generator=gen)]


def assert_f32_exact(*ts):
    """Every value an integer of magnitude < 2**24: exactly representable in f32."""
    for t in ts:
        t = t.to(F64)
        assert bool((t == t.round()).all()), "not an integer grid"
        m = float(t.abs().max()) if t.numel() else 0.0
        assert m < LIMIT, m


def lo_half_input(shape, gen):
    """k / 16 for integer |k| <= 4095 with random signs: exact in f32 and as bf16 hi + bf16 lo,
    but not in one bf16 — conv1 input values for the fused weight gradient's lo half."""
    k = torch.randint(0, 4096, tuple(shape), generator=gen).to(F64)
    s = torch.randint(0, 2, tuple(shape), generator=gen).to(F64) * 2 - 1
    return k * s / 16


# geometry list of the kernel tests: id -> (B, T1, F1, C), (T1, F1) the conv1 output grid
GEOMETRIES = {
    "g_min": (1, 3, 3, 64),
    "g_even": (2, 4, 4, 64),
    "g_f4": (3, 30, 9, 64),
    "g_f19": (2, 7, 39, 64),
    "g_f19e": (2, 9, 40, 64),
    "g_f33": (1, 5, 67, 64),
    "g_f63": (1, 5, 128, 64),
    "g_rows": (5, 21, 11, 64),
    "g_fwd": (3, 25, 19, 64),
    "g_c128": (2, 9, 9, 128),
    "g_c512": (2, 9, 9, 512),
    "g_c1024": (1, 7, 7, 1024),
}


class ConvCase:
    """Integer-grid inputs of one geometry and every exact reference the kernel tests need,
    all float64 on the CPU.  x: conv1 input (B, T, Fin) with T = 2*T1 + 1 + (T1 even),
    Fin likewise — an even T1 / F1 gets the one extra input row / column only the unread x1
    row / column sees."""

    def __init__(self, B, T1, F1, C, seed=0, x_values=range(-2, 3), zeros=0, lo_half=False):
        g = torch.Generator().manual_seed(seed)
        self.B, self.T1, self.F1, self.C = B, T1, F1, C
        self.T2, self.F2 = down(T1), down(F1)
        self.P1, self.P2 = B * T1 * F1, B * self.T2 * self.F2
        self.T, self.Fin = 2 * T1 + 1 + (T1 % 2 == 0), 2 * F1 + 1 + (F1 % 2 == 0)
        self.x1 = int_grid((B, T1, F1, C), (0, 1, 2), g, zeros)
        self.W2 = int_grid((C, C, 3, 3), (-1, 0, 1), g, zeros)
        self.b2 = int_grid((C,), (-1, 0, 1), g)
        self.dY2 = int_grid((B, self.T2, self.F2, C), (-1, 0, 1), g, zeros)
        self.x = int_grid((B, self.T, self.Fin), x_values, g)
        if lo_half:  # real-valued conv1 input: dw1 / db1 are then float64 results, not exact ones
            self.x = lo_half_input((B, self.T, self.Fin), g)
        # exact results
        self.fwd = conv2_fwd_ref(self.x1, self.W2)
        self.y2 = bf(torch.relu(self.fwd + self.b2))
        self.dx1 = conv2_dgrad_ref(self.x1, self.W2, self.dY2)
        self.dw2 = conv2_wgrad_ref(self.x1, self.dY2)
        self.g = bf(self.dx1)                                    # what the fused epilogue multiplies
        self.dw1, self.db1 = conv1_wgrad_ref(self.x, self.g)

    def magnitudes(self):
        """The same references on the inputs' magnitudes (ReLU mask all ones): a bound on every
        partial sum of every result in any summation order."""
        ax1, aW2, adY, ax = self.x1.abs(), self.W2.abs(), self.dY2.abs(), self.x.abs()
        fwd = conv2_fwd_ref(ax1, aW2) + self.b2.abs()
        dx1 = conv2_dgrad_ref(torch.ones_like(ax1), aW2, adY)
        dw2 = conv2_wgrad_ref(ax1, adY)
        dw1, db1 = conv1_wgrad_ref(ax, bf(dx1))
        return fwd, dx1, dw2, dw1, db1

    def check_exact(self, prefill=0):
        """The |v| < 2**24 condition for every input, intermediate and result (plus an integer
        prefill the accumulating outputs start from)."""
        assert_f32_exact(self.x1, self.W2, self.b2, self.dY2, self.x, self.fwd, self.dx1, self.g, self.dw2,
                         self.dw1, self.db1)
        assert_f32_exact(*[m + prefill for m in self.magnitudes()])


_CASES = {}


def conv_case(gid):
    """The shared, read-only ConvCase of a geometry id."""
    if gid not in _CASES:
        _CASES[gid] = ConvCase(*GEOMETRIES[gid], seed=sorted(GEOMETRIES).index(gid))
    return _CASES[gid]
