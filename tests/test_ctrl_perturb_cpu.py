"""Host side of sde_ctrl_noise / sde_ctrl_dropout in log-variance training (no GPU): coefficient columns 12-15 (include/sdeng.h), the
loss's table cache, and what is refused before any launch."""
import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.eq.sdes import VP, PinnedBM, ScaledBM
from sde_sampler_lrds_amd.losses import oc
from sde_sampler_lrds_amd.models.mlp import FourierMLP
from sde_sampler_lrds_amd.models.reparam import ClippedCtrl


def _ts(N=12, T=1.0, start=0.0):
    return torch.linspace(start, T, N + 1)


_VP = lambda: VP(0.1, 10.0, 1.0, terminal_t=1.0)  # noqa: E731
_T_MINUS_S, _S = (lambda s, T: T - s), (lambda s, T: s)
# case -> (table kind, sde, time grid, other table options, the time the loss hands its control at step k: generative_and_sde_ctrl(T - s, x) or (s, x))
CASES = {
    "em": ("em", _VP, _ts(), dict(with_ref=True), _T_MINUS_S),
    "ei": ("ei", _VP, _ts(), dict(with_ref=True), _T_MINUS_S),
    "ddpm": ("ddpm", _VP, _ts(start=1e-4, T=1.0 - 1e-4), dict(with_ref=True), _T_MINUS_S),
    "dis_ei": ("dis_ei", _VP, _ts(), {}, _T_MINUS_S),
    "time_reversal": ("time_reversal", _VP, _ts(), dict(train=True, dim=3), _S),
    "pis_scaled_bm": ("em", lambda: ScaledBM(diff_coeff=0.2 ** 0.5, terminal_t=5.0), _ts(T=5.0), {}, _T_MINUS_S),
    "ei_pinned_bm": ("ei", lambda: PinnedBM(diff_coeff=0.2 ** 0.5, terminal_t=5.0), _ts(start=1e-3, T=5.0 - 1e-3), {}, _T_MINUS_S),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_perturbation_columns_hold_sigma_p_and_the_sde_at_the_control_time(case):
    """Columns 12-15 = sigma, p, drift_coeff_t(tau_k), diff_coeff_t(tau_k) of the loss's SDE at the time its control is evaluated; columns 0-11
    bit-equal to the table without the options, whose columns 12-15 stay zero."""
    kind, make_sde, ts, kw, tau_of = CASES[case]
    sde = make_sde()
    tab = E.coef_table(kind, ts, sde, ctrl_noise=0.25, ctrl_dropout=0.6, **kw)
    plain = E.coef_table(kind, ts, sde, **kw)
    assert torch.equal(tab[:, :12], plain[:, :12]) and not plain[:, 12:].any()
    assert torch.all(tab[:, 12] == torch.tensor(0.25, dtype=torch.float32)) and torch.all(tab[:, 13] == torch.tensor(0.6, dtype=torch.float32))
    for k in range(ts.numel() - 1):
        tau = tau_of(ts[k], ts[-1])
        assert tab[k, 14] == sde.drift_coeff_t(tau) and tab[k, 15] == sde.diff_coeff_t(tau), (case, k)


def test_dds_table_carries_sigma_without_an_sde():
    ts = _ts()
    tab = E.coef_table("dds", ts, None, alpha=1.0, sigma=1.0, ctrl_noise=0.1)
    plain = E.coef_table("dds", ts, None, alpha=1.0, sigma=1.0)
    assert torch.equal(tab[:, :12], plain[:, :12]) and torch.all(tab[:, 12] == torch.tensor(0.1)) and not tab[:, 13:].any()
    with pytest.raises(ValueError, match="linear"):
        E.coef_table("dds", ts, None, alpha=1.0, sigma=1.0, ctrl_dropout=0.5)


def test_noising_tables_refuse_the_perturbation():
    with pytest.raises(E.UnsupportedByEngine):
        E.coef_table("eubo_ei", _ts(), VP(0.1, 10.0, 1.0, terminal_t=1.0), with_ref=True, ctrl_noise=0.1)


def _ctrl(d=3):
    return ClippedCtrl(base_model=FourierMLP(dim=d, activation=torch.nn.GELU(), num_layers=4, channels=64), clip_model=1e4)


def test_coefficient_cache_rekeys_on_sigma_and_p():
    ctrl = _ctrl()
    loss = oc.EIReferenceSDELoss(ctrl, ctrl, sde=VP(0.1, 10.0, 1.0, terminal_t=1.0), method="lv", reference_ctrl=None)
    ts = _ts()
    a = loss._coef(ts, "cpu", with_ref=False, ctrl_noise=0.1)
    b = loss._coef(ts, "cpu", with_ref=False, ctrl_noise=0.2)
    c = loss._coef(ts, "cpu", with_ref=False, ctrl_noise=0.2, ctrl_dropout=0.5)
    d = loss._coef(ts, "cpu", with_ref=False)
    assert float(a[0, 12]) == pytest.approx(0.1) and float(b[0, 12]) == pytest.approx(0.2)
    assert float(c[0, 13]) == 0.5 and float(b[0, 13]) == 0.0 and not d[:, 12:].any()
    assert loss._coef(ts, "cpu", with_ref=False, ctrl_noise=0.1)[0, 12] == a[0, 12]


def test_lv_options_map_to_table_options_and_flags():
    ctrl = _ctrl()
    loss = oc.EMReferenceSDELoss(ctrl, ctrl, sde=VP(0.1, 10.0, 1.0, terminal_t=1.0), method="lv", sde_ctrl_noise=0.3)
    assert loss._ctrl_perturbation() == {"ctrl_noise": 0.3}
    loss.sde_ctrl_dropout = 0.9
    assert loss._ctrl_perturbation() == {"ctrl_noise": 0.3, "ctrl_dropout": 0.9}
    loss.sde_ctrl_noise = loss.sde_ctrl_dropout = None
    assert loss._ctrl_perturbation() == {}
    assert (L.FLAG_CTRL_NOISE, L.FLAG_CTRL_DROPOUT) == (128, 256) and L.ABI_VERSION == 4


def test_dds_dropout_is_refused_before_anything_runs():
    """DDS has no loss-level SDE (sde=None): the reference's -sde.drift / sde.diff fails there; here a clear ValueError, before any launch."""
    ctrl = _ctrl(2)
    loss = oc.ExponentialIntegratorSDELoss(ctrl, ctrl, sde=None, method="lv", alpha=1.0, sigma=1.0, sde_ctrl_dropout=0.5)
    with pytest.raises(ValueError, match="sde=None"):
        loss(_ts(), torch.zeros(4, 2), lambda x: x.sum(-1), lambda x: x.sum(-1))
