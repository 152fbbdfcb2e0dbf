"""Decoding under soft evidence on the GPU (`HipCircuit.soft_mpe`, `HipCircuit.sample_soft`, cirkit_amd/soft_decode.py,
cirkit_amd/csrc/ck_soft_decode.hip; DESIGN.md section 11, "Decoding under soft evidence").

The reference has no such query.  The fp64 restatement of both contracts (tests/soft_decode_restatement.py) is pinned on the
CPU against brute force (tests/test_soft_decode_restatement.py); here the GPU is compared with it, item for item outside
the rows it flags `near` (a maximum that wins by less than 1e-4, a uniform within 1e-5 of a CDF boundary) -- at most 5 % of
the rows, which the CPU test asserts on these very inputs (`parity_inputs`).

Value tolerance, the project's rule: ``max |got - want| / (1 + |want|)`` over the finite ``want`` within 4 x the same figure
of the restatement run in fp32 on the same inputs (capped at 1e-4), at least 1e-6; printed before it is asserted; -inf meets
-inf.  Measured yardsticks and GPU errors: DESIGN.md section 11, "Decoding under soft evidence".
"""
import numpy as np
import pytest
import torch

from soft_decode_restatement import sample_soft_restated, soft_mpe_restated
from test_mpe import _deterministic_case, _hc
from test_mpe import _worlds as _all_worlds
from test_posterior_marginals import _states
from test_sampling_conditional import KAT, _chi2_p
from test_soft_decode_restatement import (NEAR_CAP, NEW_ENTRY_POINTS, NO_ROW_LEFT_OUT, PARITY_CASES, SEED, _log_worlds,
                                           parity_inputs)
from test_soft_evidence import CAP, ROWS, _plan, _soft, evidence, hard_evidence, rel_error, to_device


def _discrete(plan) -> np.ndarray:
    return _states(plan) > 0


def _sentinel(v: np.ndarray) -> np.ndarray:
    return np.isnan(v) | (v < 0)


def _rows_differ(plan, out, ch, ro, rch, gauss_too: bool) -> np.ndarray:
    """(B,) rows where a discrete value or a choice differs (`gauss_too`: or a Gaussian value, beyond 1e-5 (1 + |b|))."""
    disc = _discrete(plan)
    out = out.cpu().numpy().astype(np.float64)
    diff = ((out[:, disc] != ro[:, disc]) & ~(np.isnan(out[:, disc]) & np.isnan(ro[:, disc]))).any(axis=1)
    if gauss_too and (~disc).any():
        a, b = out[:, ~disc], ro[:, ~disc]
        diff |= ~((np.abs(a - b) <= 1e-5 * (1 + np.abs(b))) | (np.isnan(a) & np.isnan(b))).all(axis=1)
    for a, b in zip(ch, rch):
        diff |= (a.cpu().numpy() != b).any(axis=0)
    return diff


def _value_bound(plan, tensors, ll, x, soft, want) -> float:
    y32 = soft_mpe_restated(plan, tensors, ll, x, soft, dtype=np.float32)[2]
    yard = rel_error(y32, want)
    print(f"  fp32-restatement yardstick of the value: {yard:.3e}")
    return max(4 * min(yard, CAP), 1e-6)


def _check_value(got: torch.Tensor, want: np.ndarray, bound: float, what: str) -> float:
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == -np.inf, want == -np.inf)
    assert not (got == np.inf).any()
    e = rel_error(got, want)
    print(f"  GPU {what} error {e:.3e} (bound {bound:.3e})")
    assert e <= bound, (e, bound)
    return e


def _check_mpe(plan, tensors, ll, x, soft, res, rows=slice(None), ref=None):
    out, ch, lv = res
    ro, rch, rlv, near = ref if ref is not None else soft_mpe_restated(plan, tensors, ll, x, soft)
    ro, rch, rlv, near = ro[rows], [c[:, rows] for c in rch], rlv[rows], near[rows]
    if x is not None:  # observed entries: the evidence, exactly
        hard = ~np.isnan(x[rows])
        hard[:, soft] = False
        assert (out.cpu().numpy().astype(np.float64)[hard] == x[rows][hard]).all()
    diff = _rows_differ(plan, out, ch, ro, rch, gauss_too=True)
    print(f"  soft_mpe: {int(diff.sum())} differing rows, {int(near.sum())} near of {len(near)}")
    if rows == slice(None):  # (asserted on the CPU as well: tests/test_soft_decode_restatement.py)
        assert near.mean() <= NEAR_CAP
    assert not (diff & ~near).any(), np.nonzero(diff & ~near)[0][:8]
    live = np.isfinite(rlv)
    filled = out.cpu().numpy()[:, soft]
    assert (filled[live] >= 0).all() and _sentinel(filled[~live]).all()
    return rlv


def _check_sample(plan, tensors, ll, x, soft, seed, res, rows=slice(None), ref=None, leave_near_out=True):
    out, ch, le = res
    ro, rch, near, rle = ref if ref is not None else sample_soft_restated(plan, tensors, ll, x, soft, seed)
    ro, rch, near, rle = ro[rows], [c[:, rows] for c in rch], near[rows], rle[rows]
    if x is not None:
        hard = ~np.isnan(x[rows])
        hard[:, soft] = False
        assert (out.cpu().numpy().astype(np.float64)[hard] == x[rows][hard]).all()
    diff = _rows_differ(plan, out, ch, ro, rch, gauss_too=False)
    draws = sum(l.num_folds for l in plan.layers if l.type not in ("hadamard", "kronecker"))
    print(f"  sample_soft: {int(diff.sum())} differing rows, {int(near.sum())} near of {len(near)}, {draws} draws per row")
    if leave_near_out:
        if rows == slice(None):
            assert near.mean() <= NEAR_CAP
        assert not (diff & ~near).any(), np.nonzero(diff & ~near)[0][:8]
    assert diff.mean() <= max(1e-3, 2e-5 * draws), (diff.mean(), draws)
    disc = _discrete(plan)
    if (~disc).any():
        ok = ~diff
        a, b = out.cpu().numpy().astype(np.float64)[ok][:, ~disc], ro[ok][:, ~disc]
        assert (np.isnan(a) == np.isnan(b)).all()
        a, b = a[~np.isnan(b)], b[~np.isnan(b)]
        assert (np.abs(a - b) <= 1e-4 * (1 + np.abs(b))).all()
    live = np.isfinite(rle)
    filled = out.cpu().numpy()[:, soft]
    assert (filled[live] >= 0).all() and _sentinel(filled[~live]).all()
    lev = le.cpu().numpy()
    assert np.array_equal(np.isnan(lev), np.isnan(rle)) and np.array_equal(lev == -np.inf, rle == -np.inf)


def _check_leaf_bits(hc, ll_d, x_d, soft) -> int:
    """The decode leaf's maximum is the unit value the max leaf stored, bit for bit.  Right after a one-chunk `soft_mpe`, whose
    MPE arena still holds the upward values: the argmax walk is run again into a node buffer of the test's own, and at every
    recorded node (fold g, unit k) the returned state c must give table[c, k] + log_lik[n, s, c] -- one fp32 add, in torch --
    equal to the arena's value of that unit; every soft fold's whole block must equal torch's max over the states of that
    sum.  Returns the number of nodes checked."""
    from cirkit_amd import _capi as capi
    from cirkit_amd.soft_decode import _state

    st, ids = _state(hc, ll_d, x_d, soft)
    s, m = st.s, st.mpe
    q, d = st._set(ids)
    xm, ll32 = st.soft._evidence(ll_d, x_d, ids)
    B, S = int(ll32.shape[0]), int(ll32.shape[1])
    assert B in m._arenas
    arena, val_off, bases = m._arena(B)
    dev = ll32.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    node = torch.full((B, S), -1, dtype=torch.int32, device=dev)
    out, val = xm.clone(), torch.empty(B, dtype=torch.float32, device=dev)
    bad = torch.zeros(B, dtype=torch.int32, device=dev)
    capi.call("ck_soft_mpe_walk", s._table.data_ptr(), m._logw_tab.data_ptr(), m._amax_tab.data_ptr(), d["spos_tab"].data_ptr(),
              len(s.layers), s.root_fold, 0, s.total_folds, s.S, arena.data_ptr(), val_off.data_ptr(), bad.data_ptr(), 0, B, B,
              s.D, S, node.data_ptr(), xm.data_ptr(), out.data_ptr(), 1 if s.float_out else 0, val.data_ptr(), stream)
    st.decode_leaf(0, q, d, ll32, node, 0, B, 0, out, stream)
    checked = 0
    for j, sp in q["spos"].items():
        lay = s._z_circuit().layers[j]
        F, K, C = lay.num_folds, lay.num_output_units, lay.num_categories
        tab = lay._table  # (F, C + 1, K)
        stored = arena[bases[j] : bases[j] + F * B * K].view(F, B, K)
        for f in torch.nonzero(sp >= 0)[:, 0].tolist():
            si = int(sp[f])
            lv = ll32[:, si, :C]  # (B, C)
            assert torch.equal((tab[f, :C][None] + lv[:, :, None]).max(1).values, stored[f]), (j, f)
            g = int(s.fold_off[j]) + f
            on = torch.nonzero(node[:, si] // 32768 == g)[:, 0]
            if on.numel() == 0:
                continue
            k = (node[on, si] % 32768).long()
            c = out[on, int(d["vars"][si])].long()
            assert torch.equal(tab[f, c, k] + lv[on, c], stored[f, on, k]), (j, f)
            checked += int(on.numel())
    return checked


def _both(hc, ll_d, x_d, soft, seed, **kw):
    m = hc.soft_mpe(ll_d, x_d, soft_vars=soft, return_choices=True, return_log_value=True, **kw)
    s = hc.sample_soft(ll_d, x_d, soft_vars=soft, seed=seed, return_choices=True, return_log_evidence=True, **kw)
    return m, s


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                          b.view(torch.int32) if b.dtype == torch.float32 else b))


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.gpu
def test_soft_decode_surface(hip_device):
    from cirkit_amd import _capi as capi
    from cirkit_amd.circuit import HipCircuit

    lib = capi.load()
    for n in NEW_ENTRY_POINTS:
        assert hasattr(lib, n) and n in capi.SIGNATURES
    assert lib.ck_abi_version() == 51
    assert callable(HipCircuit.soft_mpe) and callable(HipCircuit.sample_soft)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", PARITY_CASES)
def test_gpu_soft_decode_equals_restatement(hip_device, name, kind):
    """Completions, draws and choices item for item outside the `near` rows; the value within the yardstick's bound; the
    log evidence bit for bit `soft_evidence_log_prob`'s.  On cfg2_qt784 nearly every row holds a `near` draw (the CPU test
    says why), so no row of `sample_soft` is left out there: the share of differing rows is bounded over all of them.  On the 256-state plans the decode
    leaf's maximum is also held, bit for bit, against the unit value the max leaf stored (`_check_leaf_bits`)."""
    plan, tensors, soft, ll, x, seed = parity_inputs(name, kind)
    hc = _hc(plan, tensors, hip_device)
    B = ll.shape[0]
    ll_d, x_d = torch.from_numpy(ll).to(hip_device), to_device(plan, x, hip_device)
    m, s = _both(hc, ll_d, x_d, soft, seed)
    if name.startswith("cat256"):  # (K = 32 / 64, C = 256: the vectorised staging of the max leaf, the 64-lane decode leaf)
        nodes = _check_leaf_bits(hc, ll_d, x_d, soft)
        print(f"  decode leaf against the stored unit values, bit for bit, at {nodes} nodes")
        assert nodes >= (B - B // 3 - 1) * len(soft)
    gauss = not _discrete(plan).all()
    for out in (m[0], s[0]):
        assert out.shape == (B, plan.num_variables) and out.dtype == (torch.float32 if gauss else torch.int64)
    sums = [j for j, l in enumerate(plan.layers) if l.type in ("sum", "cpt", "tucker")]
    for ch in (m[1], s[1]):
        assert len(ch) == len(sums)
        assert all(c.dtype == torch.int32 and tuple(c.shape) == (plan.layers[j].num_folds, B) for c, j in zip(ch, sums))
    ref_m = soft_mpe_restated(plan, tensors, ll, x, soft)
    ref_s = sample_soft_restated(plan, tensors, ll, x, soft, seed)
    _check_mpe(plan, tensors, ll, x, soft, m, ref=ref_m)
    _check_value(m[2], ref_m[2], _value_bound(plan, tensors, ll, x, soft, ref_m[2]), "value")
    _check_sample(plan, tensors, ll, x, soft, seed, s, ref=ref_s, leave_near_out=name not in NO_ROW_LEFT_OUT)
    lp = hc.soft_evidence_log_prob(ll_d, x_d, soft_vars=soft)[:, 0, 0].contiguous()
    assert _same_bits(s[2], lp)
    dead = ~np.isfinite(ref_m[2])
    assert dead.any() == (kind == "dead")
    if name.startswith("cat") and kind == "dense":  # the other row counts (ragged row tiles): the same rows, on their own
        for n in ROWS[:-1]:
            m, s = _both(hc, ll_d[:n], x_d[:n], soft, seed)
            _check_mpe(plan, tensors, ll, x, soft, m, rows=slice(0, n), ref=ref_m)
            _check_sample(plan, tensors, ll, x, soft, seed, s, rows=slice(0, n), ref=ref_s)
    hc.check_inputs()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.gpu
@pytest.mark.parametrize("name", KAT)
def test_gpu_sample_soft_draws_the_exact_posterior(hip_device, name):
    """2^20 rows under one evidence against the brute-force posterior over the 32 worlds: three soft variables, one missing,
    one observed."""
    plan, tensors = _plan(name)
    hc = _hc(plan, tensors, hip_device)
    N = 1 << 20
    w = _all_worlds(5, 2)
    y = _log_worlds(plan, tensors, w)
    soft = [0, 1, 3]
    for kind in ("dense", "three"):
        ll1 = evidence(plan, tensors, soft, 1, kind, seed=31)
        x = torch.full((N, 5), -1, dtype=torch.int64, device=hip_device)
        x[:, 4] = 1
        ll_d = torch.from_numpy(ll1).to(hip_device).expand(N, -1, -1)
        out = hc.sample_soft(ll_d, x, soft_vars=soft, seed=13)
        lw = y + sum(ll1[0, s, w[:, v]] for s, v in enumerate(soft))
        lw = np.where(w[:, 4] == 1, lw, -np.inf)
        p = np.zeros(32)
        p[w @ (1 << np.arange(5)[::-1])] = np.exp(lw) / np.exp(lw).sum()
        assert bool((out[:, 4] == 1).all()) and bool((out >= 0).all())
        got = (out * torch.tensor([16, 8, 4, 2, 1], device=hip_device)).sum(1).cpu().numpy()
        assert _chi2_p(np.bincount(got, minlength=32), p * N) >= 1e-6, kind


@pytest.mark.gpu
def test_gpu_soft_mpe_is_the_brute_force_argmax_on_a_deterministic_circuit(hip_device):
    plan, tensors = _deterministic_case()
    hc = _hc(plan, tensors, hip_device)
    w = _all_worlds(6, 4)
    y = _log_worlds(plan, tensors, w)
    soft = list(range(6))
    B = ROWS[1]
    ll = evidence(plan, tensors, soft, B, "dense", seed=32)
    out, lv = hc.soft_mpe(torch.from_numpy(ll).to(hip_device), soft_vars=soft, return_log_value=True)
    # The decode leaf's maximum is the unit value the max leaf stored, bit for bit: every fold has one unit here, so the node of
    # variable v is (its fold, unit 0), and the returned state's table entry plus log_lik must be the arena's value.
    from cirkit_amd import _capi as capi

    s = hc._sampler
    (j,) = [j for j, d in enumerate(s.layers) if d["kind"] == capi.CK_SAMPLE_CATEGORICAL]
    d, tab = s.layers[j], s._z_circuit().layers[j]._table  # (F, C + 1, 1)
    arena, _, bases = s._mpe._arena(B)
    assert d["Ko"] == 1
    stored = arena[bases[j] : bases[j] + d["F"] * B].view(d["F"], B)
    ll32 = torch.from_numpy(ll).to(hip_device).to(torch.float32)
    for f, v in enumerate(d["scope"].tolist()):
        c = out[:, v]
        got = tab[f, c, 0] + ll32[:, soft.index(v)].gather(1, c[:, None])[:, 0]
        assert torch.equal(got, stored[f]), (f, v)
        assert torch.equal((tab[f, : tab.shape[1] - 1, 0][None] + ll32[:, soft.index(v)]).max(1).values, stored[f])
    out, lv = out.cpu().numpy(), lv.cpu().numpy()
    for n in range(B):
        tot = y + sum(ll[n, s, w[:, v]] for s, v in enumerate(soft))
        top = np.sort(tot)[-2:]
        if top[1] - top[0] >= 1e-4:  # (a runner-up within the fp32 rounding of the value may win on the device)
            assert (out[n] == w[np.argmax(tot)]).all(), n
        assert abs(lv[n] - tot.max()) <= 1e-5 * (1 + abs(tot.max()))


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plan_quadgraph_1x4x4_cp", "binomial_qg6x6_k4", "cat256_k32"])
def test_gpu_soft_decode_identities(hip_device, name):
    """One-hot evidence returns its states; weight 1 everywhere is `mpe` / `sample_conditional` with the soft variables
    queried; 0 / -inf on a box keeps every draw and completion inside it."""
    plan, tensors = _plan(name)
    D, B = plan.num_variables, ROWS[-1]
    states = _states(plan)
    hc = _hc(plan, tensors, hip_device)
    soft = _soft(plan)[::2]
    S, C = len(soft), int(states[soft].max())
    rng = np.random.default_rng(7)
    x = rng.integers(0, states, size=(B, D))
    x[rng.random((B, D)) < 1 / 9] = -1
    x_d = torch.from_numpy(x).to(hip_device)
    xs = np.where(x < 0, np.nan, x.astype(np.float64))
    c = np.arange(C)[None, None, :]
    # one-hot at y
    yv = rng.integers(0, states[soft], size=(B, S))
    ll = np.where(c == yv[:, :, None], 0.0, -np.inf)
    ll_d = torch.from_numpy(ll).to(hip_device)
    (mo, _, mv), (so, _, sv) = _both(hc, ll_d, x_d, soft, SEED)
    live = torch.isfinite(sv)
    assert bool(live.any()) and bool((torch.isfinite(mv) == live).all())
    y_d = torch.from_numpy(yv).to(hip_device)
    assert bool((mo[:, soft][live] == y_d[live]).all()) and bool((so[:, soft][live] == y_d[live]).all())
    xy = x.copy()
    xy[:, soft] = yv
    _, want = hc.mpe(torch.from_numpy(xy).to(hip_device), [], return_log_value=True)  # (the sentinels of x are maximised)
    ref = soft_mpe_restated(plan, tensors, ll, xs, soft)
    bound = _value_bound(plan, tensors, ll, xs, soft, ref[2])
    _check_value(mv, want.cpu().numpy().astype(np.float64), bound, "one-hot value against mpe")
    # weight 1 everywhere
    zero = torch.zeros((B, S, C), device=hip_device)
    (mo, mc, mv), (so, sc, sv) = _both(hc, zero, x_d, soft, SEED)
    ho, hc_, hv = hc.mpe(x_d, soft, return_choices=True, return_log_value=True)
    _, _, _, near = soft_mpe_restated(plan, tensors, np.zeros((B, S, C)), xs, soft)
    differ = (mo != ho).any(1).cpu().numpy()
    for a, b in zip(mc, hc_):
        differ |= (a != b).any(0).cpu().numpy()
    assert not (differ & ~near).any()
    co = hc.sample_conditional(x_d, soft, seed=SEED)
    agree = (co == so).all(1).float().mean().item()
    print(f"  sample_soft(log_lik = 0) equals sample_conditional in {agree:.4f} of the rows")
    assert agree > 0.98
    # 0 inside [lo, hi], -inf outside
    a, b = rng.integers(0, states[soft], size=(B, S)), rng.integers(0, states[soft], size=(B, S))
    a, b = np.minimum(a, b), np.maximum(a, b)
    ll = np.where((c >= a[:, :, None]) & (c <= b[:, :, None]), 0.0, -np.inf)
    ll_d = torch.from_numpy(ll).to(hip_device)
    (mo, _, mv), (so, _, sv) = _both(hc, ll_d, x_d, soft, SEED)
    a_d, b_d = torch.from_numpy(a).to(hip_device), torch.from_numpy(b).to(hip_device)
    live = torch.isfinite(sv)
    assert bool(live.all()) and bool(torch.isfinite(mv).all())
    for o in (mo, so):
        assert bool(((o[:, soft] >= a_d) & (o[:, soft] <= b_d)).all())
    lo, hi = x.copy(), x.copy()
    lo[:, soft], hi[:, soft] = a, b
    box = hc.interval_log_prob(torch.from_numpy(lo).to(hip_device), torch.from_numpy(hi).to(hip_device))[:, 0, 0]
    from test_soft_evidence import Reference

    r = Reference(plan, tensors, ll, xs, soft)
    e = rel_error(sv.cpu().numpy(), box.cpu().numpy().astype(np.float64))
    print(f"  log evidence against interval_log_prob {e:.3e} (bound {r.bound:.3e})")
    assert e <= r.bound
    hc.check_inputs()


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["hazard_onehot", "hazard_channel"])
@pytest.mark.parametrize("name", ["binomial_qg6x6_k4", "cat256_k32"])
def test_gpu_soft_decode_where_the_table_is_in_a_far_tail(hip_device, name, kind):
    """Evidence centred on each variable's least likely state (Binomial-255 log-pmf tables, 256-state softmax rows with logit
    standard deviation 30): both leaves stay in log space, so no value is -inf where the restatement is finite and, under
    one-hot evidence, every row returns the one live state."""
    plan, tensors = _plan(name, logit_std=30.0) if name == "cat256_k32" else _plan(name)
    hc = _hc(plan, tensors, hip_device)
    B = ROWS[1]
    soft = _soft(plan)
    ll = evidence(plan, tensors, soft, B, kind, seed=6)
    ref = soft_mpe_restated(plan, tensors, ll, None, soft)
    assert np.isfinite(ref[2]).all()
    (mo, _, mv), (so, _, sv) = _both(hc, torch.from_numpy(ll).to(hip_device), None, soft, SEED)
    assert bool(torch.isfinite(mv).all()) and bool(torch.isfinite(sv).all())
    _check_value(mv, ref[2], _value_bound(plan, tensors, ll, None, soft, ref[2]), "value")
    if kind == "hazard_onehot":
        y = torch.from_numpy(np.argmax(ll, axis=2)).to(hip_device)
        assert bool((mo[:, soft] == y).all()) and bool((so[:, soft] == y).all())
    else:
        assert bool((mo[:, soft] >= 0).all()) and bool((so[:, soft] >= 0).all())


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plan_quadgraph_1x4x4_cp", "cat256_k32", "plan_clt_mixed6_cp"])
def test_gpu_soft_decode_bad_rows_and_chunking(hip_device, name):
    """A NaN in a read entry of one row, an out-of-range hard category in another and a dead variable in a third: exactly
    those rows keep their sentinels, with value / evidence NaN, NaN and -inf; `check_inputs` reports the second; every other
    row is unchanged; `rows_per_chunk` changes nothing, bit for bit."""
    plan, tensors = _plan(name)
    hc = _hc(plan, tensors, hip_device)
    B = ROWS[-1]
    states = _states(plan)
    soft = _soft(plan)[::2]
    hard = [v for v in range(plan.num_variables) if states[v] > 0 and v not in soft]
    ll = evidence(plan, tensors, soft, B, "dense", seed=8)
    x = hard_evidence(plan, B, seed=8)
    x[62, hard[0]] = 0
    ll_d = torch.from_numpy(ll).to(hip_device)
    clean = _both(hc, ll_d, to_device(plan, x, hip_device), soft, SEED)
    hc.check_inputs()
    assert all(bool(torch.isfinite(r[2]).all()) for r in clean)
    ll[5, 0, 1] = np.nan
    ll[40, len(soft) - 1, :] = -np.inf
    x[62, hard[0]] = states[hard[0]]
    ll_d, x_d = torch.from_numpy(ll).to(hip_device), to_device(plan, x, hip_device)
    bad_rows = torch.zeros(B, dtype=torch.bool, device=hip_device)
    bad_rows[[5, 40, 62]] = True
    soft_d = torch.tensor(soft, device=hip_device)
    res = []
    for r in (None, 7):
        m, s = _both(hc, ll_d, x_d, soft, SEED, rows_per_chunk=r)
        with pytest.raises(IndexError):
            hc.check_inputs()
        for out, _, v in (m, s):
            assert bool(torch.isnan(v[5])) and bool(torch.isnan(v[62])) and float(v[40]) == -np.inf
            assert bool(torch.isfinite(v[~bad_rows]).all())
            filled = out[:, soft_d]
            sentinel = torch.isnan(filled) if filled.dtype == torch.float32 else filled < 0
            assert bool(sentinel[bad_rows].all()) and not bool(sentinel[~bad_rows].any())
        res.append((m, s))
    for (a, ac, av), (b, bc, bv) in zip(res[0], res[1]):
        assert _same_bits(a, b) and _same_bits(av, bv) and all(torch.equal(p, q) for p, q in zip(ac, bc))
    ok = ~bad_rows
    for (a, ac, av), (b, bc, bv) in zip(res[0], clean):
        assert _same_bits(a[ok], b[ok]) and _same_bits(av[ok], bv[ok])
        assert all(torch.equal(p[:, ok], q[:, ok]) for p, q in zip(ac, bc))
    with pytest.raises(ValueError):
        hc.soft_mpe(ll_d, x_d, soft_vars=soft, rows_per_chunk=0)


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.gpu
def test_gpu_soft_decode_follows_the_parameters(hip_device):
    plan, tensors = _plan("cat256_k32")
    hc = _hc(plan, tensors, hip_device)
    soft = _soft(plan)
    B = ROWS[1]
    ll_d = torch.from_numpy(evidence(plan, tensors, soft, B, "channel", seed=9)).to(hip_device)
    before = _both(hc, ll_d, None, soft, SEED)
    cat = plan.layers[0]
    name = [n for n in cat.params["probs"].nodes if n.op == "tensor"][0].config["tensor"]
    v = np.array(hc.store.export(name), dtype=np.float32)
    v = (v + 2.0 * np.random.default_rng(10).normal(size=v.shape)).astype(np.float32)
    hc.store.set(name, v)
    tensors = dict(tensors)
    tensors[name] = v
    after = _both(hc, ll_d, None, soft, SEED)
    fresh = _both(_hc(plan, tensors, hip_device), ll_d, None, soft, SEED)
    for (a, ac, av), (b, bc, bv), (o, _, ov) in zip(after, fresh, before):
        assert not torch.equal(av, ov)
        assert _same_bits(a, b) and _same_bits(av, bv) and all(torch.equal(p, q) for p, q in zip(ac, bc))


@pytest.mark.gpu
def test_gpu_soft_decode_refusals(hip_device):
    """Raised before anything is allocated or launched: no `Sampler` exists afterwards."""
    import os

    from cirkit_amd.plan import Plan
    from cirkit_amd.initializers import init_plan_tensors
    from conftest import GOLDEN

    plan, tensors = _plan("plan_clt_mixed6_cp")  # variables 0, 2, 4 discrete (3 states), 1, 3, 5 Gaussian
    hc = _hc(plan, tensors, hip_device)
    ll = torch.zeros((4, 3, 3), device=hip_device)
    for fn in (hc.soft_mpe, hc.sample_soft):
        with pytest.raises(NotImplementedError, match="Gaussian"):
            fn(torch.zeros((4, 2, 3), device=hip_device), soft_vars=[0, 1])
        for bad_ll, bad_x, sv in [(ll[0], None, None), (ll[:, :2], None, None), (ll[:, :, :2], None, None),
                                  (ll, torch.zeros((3, 6), device=hip_device), None), (ll.long(), None, None), (ll, None, [0, 2]),
                                  (ll, None, [7])]:
            with pytest.raises(ValueError):
                fn(bad_ll, bad_x, soft_vars=sv)
        with pytest.raises(ValueError):
            fn(ll, rows_per_chunk=0)
        assert getattr(hc, "_sampler", None) is None
    sos = Plan.load(os.path.join(GOLDEN, "cfg5_sos_c_k32"))
    hs = _hc(sos, init_plan_tensors(sos), hip_device)
    for fn in (hs.soft_mpe, hs.sample_soft):
        with pytest.raises(ValueError, match="lse-sum"):
            fn(torch.zeros((4, 16, 256), device=hip_device))
        assert getattr(hs, "_sampler", None) is None
