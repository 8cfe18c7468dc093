"""The split-f16 A-operand image (csrc/image_format.hpp), decoded back into matrices by a NumPy decoder of the format that shares no code
with the package: the drift net's forward and transposed images in a VjpSession's workspace, the tilted net's slots and constants in
its cached workspace.

Format: v is stored as hi = f16(v) and lo = f16((v - hi) * 2^11); a block is one (16-output tile `to`, 32-input K-block `kb`), blocks in
the order (to, kb, part, lane, 8 halves); half j of lane l is element (16 to + l % 16, 16 (2 kb + j // 4) + 4 (l // 16) + j % 4).
A matrix whose largest finite |entry| is outside [2^-10, 2^14) is stored times 2^e, that entry in [1, 2), |e| <= 100; its bias alike.

Asserted per matrix: pad entries are exactly 0 in both parts; the stored scale is 2^e of the rule and its inverse 2^-e; with v = W 2^e in
fp32, |hi + lo / 2048 - v| <= 2^-22 |v| + 2^-36 (two round-to-nearest f16 casts, the residual exact in fp32; a subnormal lo is off by at
most 2^-25, over 2048); the bias is b 2^e bit for bit; the transposed image decodes to the transpose under the same scale."""
import math

import numpy as np
import pytest
import torch

from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.eq import sdes
from sde_sampler_lrds_amd.models import mlp, reparam
from sde_sampler_lrds_amd.models import utils as mutils
from tests import tilted_cases as tc

pytestmark = pytest.mark.gpu
DIMS = [2, 40, 100, 128]  # NT = 1, 3 (last K-block half empty), 7 (partial last tile), 8
ROWS = 16
REL, ABS = 2.0 ** -22, 2.0 ** -36
BLOCK = 512  # floats of one block


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------
def decode(floats, out_tiles, k_blocks):
    """[out_tiles * k_blocks * 512] float32 words of an image -> (hi, lo) float16 arrays [16 out_tiles, 32 k_blocks]."""
    assert floats.size == out_tiles * k_blocks * BLOCK
    halves = floats.view(np.float16).reshape(out_tiles, k_blocks, 2, 64, 8)
    to, kb, lane, j = np.meshgrid(np.arange(out_tiles), np.arange(k_blocks), np.arange(64), np.arange(8), indexing="ij")
    o, i = 16 * to + lane % 16, 16 * (2 * kb + j // 4) + 4 * (lane // 16) + j % 4
    parts = []
    for part in (0, 1):
        m = np.full((16 * out_tiles, 32 * k_blocks), np.nan, dtype=np.float16)
        m[o, i] = halves[:, :, part]
        assert not np.isnan(m).any()  # every element of the grid is some half
        parts.append(m)
    return parts


def rule_exponent(w):
    a = np.abs(w[np.isfinite(w)])
    mx = float(a.max()) if a.size else 0.0
    if mx > 0.0 and (mx < 2.0 ** -10 or mx >= 2.0 ** 14):
        return int(np.clip(1 - math.frexp(mx)[1], -100, 100))
    return 0


def check_image(tag, floats, out_tiles, k_blocks, w, e):
    """The image holds ``w`` [n_out, n_in] times 2^e."""
    hi, lo = decode(floats, out_tiles, k_blocks)
    n_out, n_in = w.shape
    pad = np.ones(hi.shape, dtype=bool)
    pad[:n_out, :n_in] = False
    assert not hi[pad].any() and not lo[pad].any(), f"{tag}: non-zero pad entry"
    v = (w.astype(np.float32) * np.float32(2.0 ** e)).astype(np.float64)
    dec = hi[:n_out, :n_in].astype(np.float64) + lo[:n_out, :n_in].astype(np.float64) / 2048.0
    ratio = float((np.abs(dec - v) / (REL * np.abs(v) + ABS)).max())
    print(f"{tag}: [{n_out} x {n_in}] in {out_tiles} x {k_blocks} blocks, e = {e}, worst |decoded - v| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{tag}: decoded value off by {ratio:.3f} of the bound"


def check_scaled(tag, got, b, e, pad_len):
    want = np.zeros(pad_len, dtype=np.float32)
    want[:b.size] = b.astype(np.float32) * np.float32(2.0 ** e)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{tag}: bias is not b * 2^e bit for bit"


def f32(t):
    return t.detach().cpu().numpy().astype(np.float32)


def words(ws):
    torch.cuda.synchronize()
    return ws.cpu().numpy().view(np.float32)


# ---- weight states -------------------------------------------------------------------------------------------------------------------
def draw_in_range_(net, g):
    """Every weight matrix spread over (-1, 1): largest entry inside [2^-10, 2^14), and 3e4 times it outside.  A product of two draws, so
    that the entries use fp32's whole mantissa (torch.rand alone yields multiples of 2^-24, which the split stores exactly)."""
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() == 2 and name != "timestep_embed.timestep_phase":
                p.copy_((2.0 * torch.rand(p.shape, generator=g) - 1.0) * (0.5 + 0.5 * torch.rand(p.shape, generator=g)))
            elif name.endswith("bias"):
                p.copy_(0.5 * torch.randn(p.shape, generator=g))


def fourier_mlp(d, state, layers, channels, seed):
    """state: 'in_range', 'default' (the reference's near-zero last layer, models/utils.py) or 'big:<module path>'."""
    torch.manual_seed(seed)
    net = mlp.FourierMLP(dim=d, activation=torch.nn.GELU(), num_layers=layers, channels=channels, last_bias_init=mutils.init_bias_uniform_zeros,
                         last_weight_init=mutils.kaiming_uniform_zeros_)
    if state != "default":
        draw_in_range_(net, torch.Generator().manual_seed(seed))
    if state.startswith("big:"):
        mod = net
        for part in state[4:].split("."):
            mod = mod[int(part)] if part.isdigit() else getattr(mod, part)
        with torch.no_grad():
            mod.weight.mul_(3e4)
            mod.bias.mul_(3e4)
    return net


def expect_sign(state, path, e):
    """in range: e = 0; the default initialisation's last layer: e > 0; the matrix times 3e4: e < 0."""
    if state == "default" and path == "out_layer":
        assert e > 0
    elif state == "big:" + path:
        assert e < 0
    else:
        assert e == 0, (state, path, e)


# ---- drift net -----------------------------------------------------------------------------------------------------------------------
DRIFT_LAYERS = ("input_embed", "hidden_layer.0", "hidden_layer.1", "out_layer")


@pytest.mark.parametrize("state", ["in_range", "default"] + ["big:" + p for p in DRIFT_LAYERS])
@pytest.mark.parametrize("d", DIMS)
def test_drift_net_images(gpu, d, state):
    net = fourier_mlp(d, state, 4, 64, 100 + d)
    ctrl = reparam.ClippedCtrl(base_model=net, clip_model=1e4).to(gpu)
    g = torch.Generator().manual_seed(d)
    session = E.VjpSession(ctrl, torch.tensor([0.4]), torch.randn(1, ROWS, d, generator=g).to(gpu))
    session.forward_u()
    ws = words(session.ws)
    NT, H = (d + 15) // 16, 64
    KB = (NT + 1) // 2
    shapes = [(4, KB), (4, 2), (4, 2), (NT, 2)]  # (output tiles, K-blocks) of W_in, W_h1, W_h2, W_out
    offs = np.cumsum([0] + [a * b * BLOCK for a, b in shapes])
    off_bias, off_scales = offs[4], offs[4] + 3 * H + 16 * NT
    off_t = (off_scales + 8 + 63) // 64 * 64  # the transposed image: behind the forward image, aligned to 64 floats
    mods = [net.input_embed, net.hidden_layer[0], net.hidden_layer[1], net.out_layer]
    W, b = [f32(m.weight) for m in mods], [f32(m.bias) for m in mods]
    es = [rule_exponent(w) for w in W]
    for l in range(4):
        expect_sign(state, DRIFT_LAYERS[l], es[l])
        assert ws[off_scales + l] == 2.0 ** es[l] and ws[off_scales + 4 + l] == 2.0 ** -es[l], f"layer {l}: stored scale against 2^{es[l]}"
        check_image(f"d={d} {state} layer {l}", ws[offs[l]:offs[l + 1]], *shapes[l], W[l], es[l])
        check_scaled(f"layer {l}", ws[off_bias + H * l:off_bias + H * l + (H if l < 3 else 16 * NT)], b[l], es[l], H if l < 3 else 16 * NT)
        # slot l of the transposed image has layer l's shape and holds the transpose of matrix 3 - l under that matrix's scale
        check_image(f"d={d} {state} transposed slot {l}", ws[off_t + offs[l]:off_t + offs[l + 1]], *shapes[l], W[3 - l].T, es[3 - l])


# ---- tilted net ----------------------------------------------------------------------------------------------------------------------
SLOT = 16384
TE1S, TE1C, TE2, WIN, WH, WOUT, WOUT_T, WH_T, WIN_T, EIG = 0, 1, 2, 3, 4, 8, 9, 10, 14, 15
C_COEFF, C_PHASE, C_BTE1, C_BTE2, C_BIN, C_BH, C_BOUT, C_MEANG, C_VARG, C_SCALE, C_INV, C_LOGW, C_MEANS = (
    0, 128, 256, 384, 512, 640, 1152, 1280, 1408, 1536, 1600, 1664, 1680)
KMAX = 16
C_VARS = C_MEANS + KMAX * 128


@pytest.mark.parametrize("state", ["in_range", "default", "big:hidden_layer.1"])
@pytest.mark.parametrize("d", DIMS)
def test_tilted_net_images(gpu, d, state):
    spec = dict(d=d, prior="eig", K=2, times=[0.5], B=ROWS, sde="vp", t_limit=0.0, st=False, seed=700 + d)
    weights, means, (D, P) = tc.draw_mixture(spec, torch.Generator().manual_seed(spec["seed"]))
    base = fourier_mlp(d, state, 6, 128, 200 + d)
    net = reparam.GMMTitledPotential(base, tc.make_sde(sdes, "vp"), weights, means, (D, P), t_limit=0.0, use_s_t_scaling=False, tilt_type="dot")
    t, x = tc.draw_inputs(spec, net)
    net = net.to(gpu).requires_grad_(False)
    E.tilted_eval(net, t.to(gpu), x.to(gpu))
    ws = words(E._TILTED_PACKS[net][1])
    K, H, HT, HKB = 2, 128, 8, 4
    NT, KBD = (d + 15) // 16, (d + 31) // 32
    cs = ws[(EIG + 2 * K) * SLOT:]

    def check(tag, slot, out_tiles, k_blocks, w, scale_of, path=None, bias=None, bias_off=None):
        e = rule_exponent(scale_of)
        if path:
            expect_sign(state, path, e)
        assert cs[C_SCALE + slot] == 2.0 ** e and cs[C_INV + slot] == 2.0 ** -e, f"{tag}: stored scale against 2^{e}"
        check_image(f"d={d} {state} {tag}", ws[slot * SLOT:slot * SLOT + out_tiles * k_blocks * BLOCK], out_tiles, k_blocks, w, e)
        if bias is not None:
            check_scaled(tag, cs[bias_off:bias_off + 128], bias, e, 128)

    te = base.timestep_embed
    w1 = f32(te.hidden_layer[0].weight)  # [128, 256]: the sine and the cosine half, one scale
    check("te1 sin", TE1S, HT, HKB, w1[:, :H], w1, bias=f32(te.hidden_layer[0].bias), bias_off=C_BTE1)
    check("te1 cos", TE1C, HT, HKB, w1[:, H:], w1)
    check("te2", TE2, HT, HKB, f32(te.out_layer.weight), f32(te.out_layer.weight), bias=f32(te.out_layer.bias), bias_off=C_BTE2)
    w_in, w_out = f32(base.input_embed.weight), f32(base.out_layer.weight)
    check("w_in", WIN, HT, KBD, w_in, w_in, "input_embed", f32(base.input_embed.bias), C_BIN)
    check("w_in^T", WIN_T, NT, HKB, w_in.T, w_in, "input_embed")
    for l in range(4):
        w = f32(base.hidden_layer[l].weight)
        check(f"w_h{l}", WH + l, HT, HKB, w, w, f"hidden_layer.{l}", f32(base.hidden_layer[l].bias), C_BH + 128 * l)
        check(f"w_h{l}^T", WH_T + l, HT, HKB, w.T, w, f"hidden_layer.{l}")
    check("w_out", WOUT, NT, HKB, w_out, w_out, "out_layer", f32(base.out_layer.bias), C_BOUT)
    check("w_out^T", WOUT_T, HT, KBD, w_out.T, w_out, "out_layer")
    for k in range(K):  # eigenvectors of component k: P^T, then P
        check(f"P{k}^T", EIG + 2 * k, NT, KBD, f32(P[k]).T, f32(P[k]))
        check(f"P{k}", EIG + 2 * k + 1, NT, KBD, f32(P[k]), f32(P[k]))
    # the constants behind the slots: copies padded to 128 features and KMAX components (variances with 1), the log of the normalised weights
    pad = lambda v, fill=0.0: np.concatenate([v, np.full(128 - v.size, fill, dtype=np.float32)])  # noqa: E731
    assert np.array_equal(cs[C_COEFF:C_COEFF + 128], f32(te.timestep_coeff).ravel()) and np.array_equal(cs[C_PHASE:C_PHASE + 128], f32(te.timestep_phase).ravel())
    assert np.array_equal(cs[C_MEANG:C_MEANG + 128], pad(f32(net.mean_gauss).ravel())) and np.array_equal(cs[C_VARG:C_VARG + 128], pad(f32(net.var_gauss).ravel()))
    for k in range(KMAX):
        mk, vk = (pad(f32(means[k])), pad(f32(D[k]), 1.0)) if k < K else (np.zeros(128, np.float32), np.ones(128, np.float32))
        assert np.array_equal(cs[C_MEANS + 128 * k:C_MEANS + 128 * (k + 1)], mk) and np.array_equal(cs[C_VARS + 128 * k:C_VARS + 128 * (k + 1)], vk)
    logw = np.log(f32(weights).astype(np.float64) / f32(weights).astype(np.float64).sum())
    assert np.allclose(cs[C_LOGW:C_LOGW + K], logw, rtol=0.0, atol=1e-6) and np.all(np.isneginf(cs[C_LOGW + K:C_LOGW + KMAX]))
