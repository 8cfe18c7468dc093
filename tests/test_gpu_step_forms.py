"""The step body of the plain mixture sampler (k_simulate, RF_GMM, PAR = 0) under each of its wave-uniform run-time forms, held BIT FOR
BIT to its PAR = 1 trajectory twin and to a rerun, at 16 steps:

* the headline form -- K = 4 over one shared variance vector (the centred table), model clip on, un-scaled net -- at d = 128 and d = 100
  (pad features in the last tile), B = 37 (one ragged tile, one wave) and B = 40 000 (every wave slot busy, two waves per SIMD, ragged
  last round; there blocks of 48 rows, one per wave slot, also equal a small launch of just that block);
* the other side of each condition: K = 3, K = 4 with distinct variances, the clip off, an output layer at the reference's
  initialisation magnitude (stored scaled), a scaled hidden layer (range-safe twin every step);
* the range guard tripping inside the loop (one entry of 1e5 in a few particles of different tiles and wave slots), a clip small enough
  to bind in some lanes, and a NaN particle, which must come out NaN with its neighbours untouched.

The clip's trip test (a maximum tree over the output group, sim_device.hpp absmax_tile) sits in every one of these paths but clip_off; its
CPU restatement is tests/test_clip_tree_cpu.py."""
import pytest
import torch

from sde_sampler_lrds_amd.experiments import baseline_configs as cfgs

N = 16


def _same(a, b):
    """bit-equal, NaN equal to NaN"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0)) and \
        torch.equal(torch.signbit(a.nan_to_num(0.0)), torch.signbit(b.nan_to_num(0.0)))


def _plain_twin_rerun(loss, ts, x0, args, kw, name):
    loss.particle0 = 0
    x, rnd, _ = loss.simulate(ts, x0, *args, **kw)
    xa, rnda, _ = loss.simulate(ts, x0, *args, **kw)
    assert _same(x, xa) and _same(rnd, rnda), f"{name}: rerun differs"
    xt, rndt, xs = loss.simulate(ts, x0, *args, return_traj=True, **kw)
    assert xs.shape[0] == ts.numel() and _same(xs[-1], xt)
    assert _same(xt, x), f"{name}: PAR=1 twin x_N differs from the plain kernel's"
    assert _same(rndt, rnd), f"{name}: PAR=1 twin log-weights differ from the plain kernel's"
    return x, rnd


def _build(gpu, B, d=128, K=4, kind="shared", seed=1):
    g = torch.Generator().manual_seed(100 * d + K)
    v = 0.3 + torch.rand(d, generator=g)
    var = 0.3 + torch.rand(K, d, generator=g) if kind == "distinct" else v.repeat(K, 1)
    loss, ts, x0, args, kw, info = cfgs.build_rds_gmm(gpu, B, N, d=d, K=K, seed=seed + d + K, ref_var=var, ref_weights=torch.arange(1.0, K + 1.0))
    loss.seed = 23
    return loss, ts, x0, args, kw, info


@pytest.mark.gpu
@pytest.mark.parametrize("d", [128, 100])
@pytest.mark.parametrize("B", [37, 40000])
def test_headline_form_against_its_twin(gpu, d, B):
    loss, ts, x0, args, kw, _ = _build(gpu, B, d=d)
    x, rnd = _plain_twin_rerun(loss, ts, x0, args, kw, f"d={d} B={B}")
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(rnd).all())
    if B < 40000:
        return
    ntiles, grid = (B + 15) // 16, 256
    for wave in range(8):  # tile = block + grid * (wave + 8 * round): one block per wave slot, straddling a tile boundary
        tile = 11 + grid * wave
        assert tile < ntiles
        lo = 16 * tile - 8
        loss.particle0 = lo
        part = loss.simulate(ts, x0[lo:lo + 48].contiguous(), *args, **kw)
        assert torch.equal(part[0], x[lo:lo + 48]) and torch.equal(part[1], rnd[lo:lo + 48]), f"wave slot {wave}"
    loss.particle0 = 0


def _scale_layer(info, which, factor):
    mod = info["ctrl"].base_model
    for part in which.split("."):
        mod = mod[int(part)] if part.isdigit() else getattr(mod, part)
    with torch.no_grad():
        mod.weight.mul_(factor)
        mod.bias.mul_(factor)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["shared_k4", "three_modes", "distinct_variances", "clip_off", "scaled_output_layer", "scaled_hidden_layer"])
def test_each_side_of_the_entry_conditions(gpu, case):
    """One case on the headline side (shared_k4), one on the other side of each condition; B = 333 (ragged), d = 100 (pad features)."""
    K = 3 if case == "three_modes" else 4
    loss, ts, x0, args, kw, info = _build(gpu, 333, d=100, K=K, kind="distinct" if case == "distinct_variances" else "shared")
    if case == "clip_off":
        info["ctrl"].clip_model = None
    if case == "scaled_output_layer":  # |w| <= 1e-7: f16-subnormal, stored times a power of two (the reference's default initialisation)
        _scale_layer(info, "out_layer", 1e-6)
        assert float(info["ctrl"].base_model.out_layer.weight.detach().abs().max()) < 2e-7
    if case == "scaled_hidden_layer":
        _scale_layer(info, "hidden_layer.0", 3e-5)
    x, rnd = _plain_twin_rerun(loss, ts, x0, args, kw, case)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(rnd).all())


@pytest.mark.gpu
def test_range_guard_trips_inside_the_loop(gpu):
    """One entry of 1e5 (beyond f16's 65 504) in a few particles of different tiles and wave slots: the guard trips at step 0 there,
    the step is evaluated through the range-safe twin, and the result is finite and equal in the plain kernel, its twin and a rerun.
    Particles of tiles without a large entry keep the bits of a run without any."""
    B, d = 16 * 256 * 3 + 9, 128  # three wave slots per workgroup in use, ragged
    loss, ts, x0, args, kw, _ = _build(gpu, B, d=d)
    base = loss.simulate(ts, x0, *args, **kw)
    rows = torch.tensor([3, 16 * 40 + 5, 16 * 256 + 1, 16 * (256 + 77) + 15, 16 * 512 + 8, B - 2])
    big = x0.clone()
    g = torch.Generator().manual_seed(9)
    big[rows, torch.randint(0, d, (len(rows),), generator=g)] = 1e5
    x, rnd = _plain_twin_rerun(loss, ts, big, args, kw, "range guard")
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(rnd).all())
    clean = torch.ones(B, dtype=torch.bool)
    for r in rows.tolist():
        clean[16 * (r // 16):16 * (r // 16) + 16] = False
    clean = clean.to(gpu)
    assert torch.equal(x[clean], base[0][clean]) and torch.equal(rnd[clean], base[1][clean])


@pytest.mark.gpu
def test_clip_that_binds_in_some_lanes(gpu):
    B, d = 333, 100
    loss, ts, x0, args, kw, info = _build(gpu, B, d=d)
    from sde_sampler_lrds_amd import engine as E
    u = E.ctrl_forward(info["ctrl"], 0.5, x0).abs()
    clip = float(u.flatten().kthvalue(int(0.9 * u.numel())).values)  # the 90 % quantile of |u|: binds in about a tenth of the elements
    assert clip > 0.0
    wide = loss.simulate(ts, x0, *args, **kw)
    info["ctrl"].clip_model = clip
    x, rnd = _plain_twin_rerun(loss, ts, x0, args, kw, "binding clip")
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(rnd).all())
    assert not torch.equal(x, wide[0]), "the clip did not bind"


@pytest.mark.gpu
def test_nan_particle_stays_nan_and_alone(gpu):
    B, d = 333, 128
    loss, ts, x0, args, kw, _ = _build(gpu, B, d=d)
    base = loss.simulate(ts, x0, *args, **kw)
    bad = x0.clone()
    bad[70, 17] = float("nan")
    x, rnd = _plain_twin_rerun(loss, ts, bad, args, kw, "NaN particle")
    assert bool(torch.isnan(x[70]).any()) and bool(torch.isnan(rnd[70]).all())
    others = torch.ones(B, dtype=torch.bool, device=gpu)
    others[70] = False
    assert bool(torch.isfinite(x[others]).all()) and bool(torch.isfinite(rnd[others]).all())
    tile = torch.zeros(B, dtype=torch.bool, device=gpu)
    tile[64:80] = True
    assert torch.equal(x[~tile], base[0][~tile]) and torch.equal(rnd[~tile], base[1][~tile])
