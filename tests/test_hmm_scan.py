"""`HipHMM.log_prob(segments=P)` -- the time-parallel forward, cirkit_amd/csrc/ck_hmm_scan.hip -- against the fp64 restatement of
the forward algorithm (tests/hmm_restatement.py), within the project's bound for log values (`_check`)."""
import numpy as np
import pytest
import torch

from conftest import load_case
from hmm_restatement import hmm_log_prob
from test_hmm import _case, _check, _model


# K: 3 is padded to 32 (and P = 2 has no middle matrix); 64 two waves and two tiles of start states; 128 the first K whose steps
# outgrow a wave's ring; 160 waves with different numbers of blocks, five tiles; 512 the largest, four blocks a wave.  B = 33: a
# second, ragged tile of real rows in segment 0.  P = 5 and 6 of T = 37: uneven segments; P = T: one step per segment.
@pytest.mark.gpu
@pytest.mark.parametrize("T,K,C,B,P,shuffled", [
    (5, 3, 3, 1, 2, False), (37, 3, 256, 33, 5, True), (37, 32, 3, 2, 37, False), (37, 64, 3, 33, 4, True),
    (37, 128, 3, 2, 6, False), (9, 160, 256, 2, 3, True), (5, 512, 3, 1, 3, False)])
def test_scan_matches_restatement(hip_device, T, K, C, B, P, shuffled):
    ordering = np.random.default_rng(T + K).permutation(T).tolist() if shuffled else None
    plan, tensors, x = _case(T, K, C, B, ordering=ordering)
    m = _model(plan, tensors, hip_device)
    _check(m.log_prob(torch.from_numpy(x).to(hip_device), segments=P), hmm_log_prob(plan, tensors, x))
    assert m.last_launches == 2


@pytest.mark.gpu
@pytest.mark.parametrize("K,C", [(3, 3), (64, 7)])
def test_scan_peaked_parameters(hip_device, K, C):
    """Logits scaled by 30 (tests/test_hmm.py::test_peaked_parameters): a linear-space or mis-scaled combine ends in 0 / 0 or
    loses the only route to a state."""
    plan, tensors, x = _case(37, K, C, 33, scale=30.0)
    want = hmm_log_prob(plan, tensors, x)
    assert float(want.min()) < -300
    _check(_model(plan, tensors, hip_device).log_prob(torch.from_numpy(x).to(hip_device), segments=6), want)


@pytest.mark.gpu
def test_scan_missing_entries_zero_mass_and_bad_category(hip_device):
    plan, tensors, x = _case(37, 64, 5, 33)
    m = _model(plan, tensors, hip_device)
    _check(m.log_prob(torch.from_numpy(x).to(hip_device), integrate_vars=[0, 5, 36], segments=4),
           hmm_log_prob(plan, tensors, x, [0, 5, 36]))
    ragged = x.copy()
    for b in range(33):  # suffixes of different lengths; row 32 loses every entry
        ragged[b, 37 - min(37, b + 5):] = -1
    got = m.log_prob(torch.from_numpy(ragged).to(hip_device), segments=4)
    _check(got, hmm_log_prob(plan, tensors, ragged))
    assert abs(float(got[32])) <= 1e-4  # (normalised parameters: nothing observed, log 1)
    # category 2 of position 3 has no mass in any state: the rows that observe it are -inf, not NaN; a category >= C is NaN
    tensors["t0"][list(plan.layers[0].scope_idx[:, 0]).index(3), :, 2] = -np.inf
    x[:, 3] = np.arange(33) % 5
    x[7, 20] = 5
    got = _model(plan, tensors, hip_device).log_prob(torch.from_numpy(x).to(hip_device), segments=4).cpu()
    want = hmm_log_prob(plan, tensors, np.where(x == 5, 0, x))
    assert bool(torch.isneginf(want[x[:, 3] == 2]).all()) and bool(torch.isnan(got[7]))
    keep = np.arange(33) != 7
    _check(got[keep], want[keep])


@pytest.mark.gpu
def test_scan_chunking_and_auto(hip_device):
    plan, tensors, x = _case(37, 64, 3, 33)
    m, xd = _model(plan, tensors, hip_device), torch.from_numpy(x).to(hip_device)
    got = m.log_prob(xd, segments=4).clone()
    for n in (1, 16):
        assert torch.equal(m.log_prob(xd, segments=4, rows_per_chunk=n), got)
        assert m.last_launches == 2 * -(-33 // n)
    _check(m.log_prob(xd, segments="auto"), hmm_log_prob(plan, tensors, x))


@pytest.mark.gpu
def test_scan_refusals(hip_device):
    plan, tensors, x = _case(5, 3, 3, 2)
    m, xd = _model(plan, tensors, hip_device), torch.from_numpy(x).to(hip_device)
    for bad in (1, 6, 0):
        with pytest.raises(ValueError):
            m.log_prob(xd, segments=bad)
    plan, tensors, g = load_case("hmm_gauss_t3_k4")
    with pytest.raises(NotImplementedError, match=r"layer \d+ \(gaussian\)"):
        _model(plan, tensors, hip_device).log_prob(torch.from_numpy(g["x"]).to(hip_device), segments=2)
    plan, tensors, x = _case(3, 544, 3, 1)
    with pytest.raises(NotImplementedError, match="544"):
        _model(plan, tensors, hip_device).log_prob(torch.from_numpy(x).to(hip_device), segments=2)
    assert m.last_launches == 0
