"""The model clip's trip test as a maximum tree (sim_device.hpp absmax_tile / clamp_tile_rare, sim_kernel.hpp out_group).

Old: every element's !(|u| <= clip) or-ed into a per-lane flag, the flags into a wave-wide ballot, and -- only when some lane tripped --
the NaN-preserving clamp on every element of the wave.  New: the lane's largest |u| from a tree of maxima that DROP NaN operands (fmaxf,
v_max3_f32), one compare per lane, the same ballot and clamp.  The two tests differ exactly where a lane's only offenders are NaNs: the new
one does not trip there.  The clamp leaves a NaN a NaN and an in-range value as it is, so the RESULT is the same, bit for bit -- held here
over random 64-lane groups with NaNs, infinities, values at +-clip and next to it, for the one-tile and the two-tile group."""
import numpy as np


def _clampf(v, m):
    """sim_device.hpp clampf: two selects, NaN compares false twice and passes through"""
    v = np.where(v < -m, -m, v)
    return np.where(v > m, m, v).astype(np.float32)


def _old(u, m):
    """u: [groups, 64 lanes, elements]"""
    lane = (~(np.abs(u) <= m)).any(axis=2)
    trip = lane.any(axis=1)
    return np.where(trip[:, None, None], _clampf(u, m), u), trip


def _absmax_tile(v, acc=None):
    a = np.abs(v)
    if acc is None:
        return np.fmax(np.fmax(np.fmax(a[..., 0], a[..., 1]), a[..., 2]), a[..., 3])
    acc = np.fmax(np.fmax(acc, a[..., 0]), a[..., 1])
    return np.fmax(np.fmax(acc, a[..., 2]), a[..., 3])


def _new(u, m):
    mx = _absmax_tile(u[..., :4])
    for o in range(1, u.shape[2] // 4):
        mx = _absmax_tile(u[..., 4 * o:4 * o + 4], mx)
    trip = (~(mx <= m)).any(axis=1)
    return np.where(trip[:, None, None], _clampf(u, m), u), trip


def _groups(rng, n, elems, clip):
    u = (rng.standard_normal((n, 64, elems)) * clip * 0.3).astype(np.float32)
    kind = rng.integers(0, 8, n)
    at = lambda k: np.flatnonzero(kind == k)  # noqa: E731
    f32 = np.float32

    def poke(rows, values, count):
        for r in rows:
            for _ in range(count):
                u[r, rng.integers(64), rng.integers(elems)] = values[rng.integers(len(values))]
    edge = [f32(clip), f32(-clip), np.nextafter(f32(clip), f32(np.inf)), np.nextafter(f32(-clip), f32(-np.inf)), np.nextafter(f32(clip), f32(0))]
    poke(at(1), [f32(np.nan)], 3)                                   # NaNs only: the old test trips, the new one does not
    poke(at(2), [f32(np.inf), f32(-np.inf), f32(3 * clip), f32(-3 * clip)], 3)
    poke(at(3), edge, 5)                                            # at the bound (in range) and one ulp beyond it
    poke(at(4), [f32(np.nan), f32(np.inf), f32(-2 * clip)] + edge, 6)  # NaNs next to real offenders, same and other lanes
    for r in at(5):                                                 # a lane that is NaN in every element
        u[r, rng.integers(64)] = np.nan
    for r in at(6):                                                 # NaN and an offender in the SAME lane
        lane = rng.integers(64)
        u[r, lane, 0], u[r, lane, elems - 1] = np.nan, -5 * clip
    u[at(7)] *= f32(1e-3)                                           # far inside, with signed zeros
    poke(at(7), [f32(0.0), f32(-0.0)], 4)
    return u


def test_max_tree_then_clamp_equals_per_element_test_then_clamp():
    rng = np.random.default_rng(42)
    for elems in (4, 8):           # clamp_tile_rare / an odd last output tile, and a pair of output tiles
        for clip in (1e4, 0.75):
            u = _groups(rng, 4000, elems, clip)
            m = np.float32(clip)
            (a, ta), (b, tb) = _old(u, m), _new(u, m)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert not (tb & ~ta).any()                      # the tree never trips where the element test did not
            only_old = ta & ~tb
            assert only_old.any()                            # ... and the NaN-only groups are in the sample
            fin = np.where(np.isnan(u[only_old]), np.float32(0), u[only_old])
            assert np.all(np.abs(fin) <= m)                  # there every non-NaN element was in range: nothing to clamp
            assert np.array_equal(np.isnan(a), np.isnan(u))  # NaNs stay NaNs, nothing else becomes one
            assert ta.any() and (~ta).any() and tb.any()
