"""Autoregressive conditionals, log probabilities, coding tables and compression of squared circuits on the GPU
(cirkit_amd/squared_autoregressive.py; the all-steps launch: `ck_squared_path_steps`, cirkit_amd/csrc/ck_sqar.hip) against fp64
enumeration (tests/squared_autoregressive_restatement.py, whose fp32 run stays below a quarter of the bound asserted here:
tests/test_squared_autoregressive_restatement.py) and, bit for bit, against the step-by-step queries the launch replaces.

Bound: ``|got - want| <= 1e-4 max(1, |want|)`` (`R.bound`) on the conditionals whose state holds at least e^-4 of its row's
largest and on the log probabilities of the (row, step) pairs whose own state does (`A.kept_states`, `A.kept_pairs`: the accuracy
caveat of "Sampling squared circuits" in DESIGN.md); a smaller state has to be finite, or -inf where the expectation is.
Identities between two GPU results use twice the bound, a sum over P steps P times.

The tiny and the 32-unit circuits are complex-valued (``complex-lse-sum``: the `TdC` kernels), the Categorical fixture is real
(``lse-sum``: the `TdR` kernels); complex PARAMETER tensors are refused by `HipSquaredCircuit` itself."""
import functools

import numpy as np
import pytest
import torch

import squared_autoregressive_restatement as A
import squared_marginal_restatement as R
import squared_sampling_restatement as S
from guarded_buffers import _Guarded, _stream

pytestmark = pytest.mark.gpu


def _held(got, want, keep, what, factor=1.0):
    f = A.frac_of_bound(got.detach().cpu(), want, keep) / factor
    print(f"{what}: worst error {f:.3f} of the bound")
    assert f <= 1.0, what
    return f


# ---- 1. tiny circuits ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_expected(sum_product):
    plan, tensors, states = R.tiny_case(sum_product)
    x = A.tiny_rows()
    return plan, tensors, x, {name: (order, A.enumerated(plan, tensors, x, order, states)) for name, order in A.tiny_orders(plan).items()}


@pytest.mark.parametrize("padded", [True, False], ids=["32units", "3units"])
@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_every_step_of_the_tiny_circuits(hip_device, sum_product, padded):
    """K = 3 (the shape-generic form) and padded to 32 units (the 32-unit form and its root), 5 rows, all 6 steps, in the default
    order, its reverse (no mixed step either) and a permutation (mixed steps)."""
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, x, want = _tiny_expected(sum_product)
    if padded:
        plan, tensors = R.pad_tiny_to_32(plan, tensors, sum_product)
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    xd = x.to(hip_device)
    total = sq.log_prob(xd).cpu().double()
    for name, (order, (_, wc, wl)) in want.items():
        cond = sq.autoregressive_conditionals(xd, None if name == "default" else order)
        assert cond.shape == (5, 6, 3) and cond.dtype == torch.float32
        assert (sq.last_mixed_launches > 0) == (name == "permuted")
        _held(cond, wc, A.kept_states(wc), f"{name}: conditionals")
        _held(torch.logsumexp(cond, dim=2), torch.zeros(5, 6), torch.ones(5, 6, dtype=torch.bool), f"{name}: rows sum to one", 2.0)
        lp = sq.autoregressive_log_probs(xd, None if name == "default" else order)
        assert lp.shape == (5, 6) and lp.dtype == torch.float32
        pairs = A.kept_pairs(wc, x, order)
        assert float(pairs.double().mean()) >= 1.0 - A.MAX_LEFT_OUT
        _held(lp, wl, pairs, f"{name}: log probabilities")
        own = xd[:, order]
        assert torch.equal(lp, cond.gather(2, own[:, :, None])[:, :, 0])  # (the same subtraction, inside the leaf)
        _held(lp.double().sum(dim=1), total, torch.ones(5, dtype=torch.bool), f"{name}: the steps sum to log_prob", 6.0)


# ---- 2. 32 signed units ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _emb32_circuit(dev, rows_per_block=1):
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, _ = R.emb32_case()
    return HipSquaredCircuit(plan, tensors, device=dev, rows_per_block=rows_per_block)


@pytest.mark.parametrize("B", [1, 3, 33])
def test_log_m_is_state_log_marginals_bit_for_bit(hip_device, B):
    """The un-normalised ``log m`` of every step equals `state_log_marginals` of that step, in the default order (one launch, no
    mixed fold), in raster order (mixed steps) and with two pixels integrated out throughout; one selected step is its column."""
    from cirkit_amd import squared_autoregressive as ar
    from cirkit_amd.squared_sampling import tree_order

    sq = _emb32_circuit(str(hip_device))
    xd = torch.from_numpy(S.golden()["emb32_x"])[:B].to(hip_device)
    default = tree_order(sq.plan)
    for name, order, gone in (("default", default, []), ("raster", S.RASTER, []), ("integrated", [v for v in default if v not in (3, 12)], [3, 12])):
        lm = ar.autoregressive_state_log_marginals(sq, xd, None if name != "raster" else order, integrate_vars=gone)
        mixed = sq.last_mixed_launches
        assert lm.shape == (B, len(order), 3)
        assert (mixed == 0) == (name == "default")
        for i, v in enumerate(order):
            ref = sq.state_log_marginals(xd, v, list(order[i + 1:]) + gone, normalized=False)
            assert torch.equal(lm[:, i], ref), f"{name}: step {i}"
        cond = sq.autoregressive_conditionals(xd, order, integrate_vars=gone)
        for i in (0, 7, len(order) - 1):
            assert torch.equal(sq.autoregressive_conditionals(xd, order, positions=[i], integrate_vars=gone)[:, 0], cond[:, i])
        some = [1, 2, 3, 9]
        assert torch.equal(sq.autoregressive_log_probs(xd, order, positions=some, integrate_vars=gone),
                           sq.autoregressive_log_probs(xd, order, integrate_vars=gone)[:, some])


def test_chunks_and_rows_per_block_do_not_change_a_bit(hip_device):
    from cirkit_amd import squared_autoregressive as ar

    sq, sq3 = _emb32_circuit(str(hip_device)), _emb32_circuit(str(hip_device), 3)
    xd = torch.from_numpy(S.golden()["emb32_x"])[:5].to(hip_device)
    for order in (None, S.RASTER):
        cond = sq.autoregressive_conditionals(xd, order).clone()
        lp = sq.autoregressive_log_probs(xd, order).clone()
        tab = sq.coding_tables(xd, order, precision=12).clone()
        for rpc in (1, 2):
            assert torch.equal(sq.autoregressive_conditionals(xd, order, rows_per_chunk=rpc), cond)
            assert torch.equal(sq.autoregressive_log_probs(xd, order, rows_per_chunk=rpc), lp)
            assert torch.equal(sq.coding_tables(xd, order, precision=12, rows_per_chunk=rpc), tab)
        for spc in (1, 5):
            assert torch.equal(ar.autoregressive_conditionals(sq, xd, order, steps_per_chunk=spc), cond)
            assert torch.equal(ar.coding_tables(sq, xd, order, precision=12, steps_per_chunk=spc, rows_per_chunk=2), tab)
        assert torch.equal(sq3.autoregressive_conditionals(xd, order), cond)
        assert torch.equal(sq3.autoregressive_log_probs(xd, order), lp)
        assert torch.equal(sq3.coding_tables(xd, order, precision=12), tab)


# ---- 3. a real circuit under lse-sum ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cat_circuit(dev):
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, _ = R.cat_case()
    return HipSquaredCircuit(plan, tensors, device=dev)


def test_real_circuit_under_lse_sum(hip_device):
    """The `sq_cat_qt4x4_k5` fixture (256 states, K = 5 padded to 32, a table of logarithms): 3 rows, all 16 steps against the
    recorded fp64 expectations; the coding tables are the numpy quantiser on the GPU's own conditionals, integer for integer."""
    sq = _cat_circuit(str(hip_device))
    g = A.golden()
    x = A.cat_rows()
    xd = x.to(hip_device)
    from cirkit_amd.squared_sampling import tree_order

    order = tree_order(sq.plan)
    wc = torch.from_numpy(g["cat_cond"])
    cond = sq.autoregressive_conditionals(xd)
    assert cond.shape == (3, 16, 256) and sq.last_mixed_launches == 0
    _held(cond, wc, A.kept_states(wc), "conditionals")
    lp = sq.autoregressive_log_probs(xd)
    _held(lp, torch.from_numpy(g["cat_logp"]), A.kept_pairs(wc, x, order), "log probabilities")
    from autoregressive_restatement import quantise

    p = torch.exp(cond).cpu().numpy().reshape(48, 256)  # (the device's exp: the host's differs in the last bit, the quantiser is an
    for precision in (10, 16, 24):  #                      integer function of the fp32 probabilities)
        tab = sq.coding_tables(xd, precision=precision)
        assert tab.shape == (3, 16, 257) and tab.dtype == torch.int32
        assert np.array_equal(tab.cpu().numpy(), quantise(p, np.full(48, 256), precision).reshape(3, 16, 257))
    assert torch.equal(sq.coding_tables(xd, positions=[4, 5, 11], precision=16), sq.coding_tables(xd, precision=16)[:, [4, 5, 11]])


# ---- 5. the kernel alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R_rows", [(1, 1), (3, 2)])
@pytest.mark.parametrize("cplx", [False, True], ids=["float", "c32"])
def test_kernel_alone_between_guard_words(hip_device, cplx, B, R_rows):
    """`ck_squared_path_steps` on the hand-built paths of `S.PATH_SHAPES`, stacked as the steps of ONE call: one and two levels,
    both kernel forms (two launches), 7, 5 and 3 states per step.  The three outputs lie between guard words: every owned word
    is written, nothing else; ``log m`` is held to `R.bound` against the fp64 restatement of each path, the columns past a step's
    C are -inf, the all -inf row (B = 3: the last row of every RANK-1 sibling) is -inf, NaN where it is normalised."""
    from cirkit_amd import _capi as capi

    dev = hip_device
    shapes = list(S.PATH_SHAPES)
    P, Cmax, e = len(shapes), S.PATH_STATES, 2 if cplx else 1
    Cs = [S.PATH_STATES, 5, 3, S.PATH_STATES, 5, 3]
    cases = [S.hand_path_case(cplx, shape, B) for shape in shapes]
    S_max = max(len(sibs) for (levels, _, _), _, _, _ in cases for _, _, _, _, sibs in levels)
    L_max = max(len(levels) for (levels, _, _), _, _, _ in cases)
    W = capi.CK_SQ_PATH_LEVEL_WORDS + 2 * S_max
    host = np.zeros((P, L_max, W), dtype=np.int64)
    leaf = np.zeros((P, capi.CK_SQ_STEP_LEAF_WORDS), dtype=np.int64)
    pools = {S.KIND_FULL: [], S.KIND_CONST: [], S.KIND_RANK1: []}
    keep = []
    D = P + 1
    x = torch.zeros((B, D), dtype=torch.int64)

    def words(t):
        t = t.to(torch.complex64 if cplx else torch.float32).contiguous()
        return (torch.view_as_real(t) if cplx else t).reshape(-1).float()

    for si, (((levels, table, tlog), _, _, _), shape) in enumerate(zip(cases, shapes)):
        for li, (st, Ki, Ko, w, sibs) in enumerate(levels):
            if st:
                wd = w.float().contiguous().to(dev)
                keep.append(wd)
                host[si, li, 0], host[si, li, 1], host[si, li, 4], host[si, li, 5] = capi.CK_SQ_PATH_STAGES, 1, wd[0].data_ptr(), wd[1].data_ptr()
            host[si, li, 2], host[si, li, 3], host[si, li, 6] = Ki, Ko if st else Ki, len(sibs)
            for h, (kd, raw, _) in enumerate(sibs):
                host[si, li, 8 + 2 * h], host[si, li, 9 + 2 * h] = kd, sum(t.numel() for t in pools[kd]) // e
                pools[kd].append(words(raw))
        td = table.float().contiguous().to(dev)
        keep.append(td)
        leaf[si] = (td[1].data_ptr(), 0, Cs[si], S.PATH_SHAPES[shape][1], tlog, si + 1, len(levels), 0)  # (fold 1, its first C states)
        x[:, si + 1] = torch.arange(B) % Cs[si]
    cat = lambda ts: torch.cat(ts).to(dev) if ts else None  # noqa: E731
    full_d, cst_d, rk_d = cat(pools[S.KIND_FULL]), cat(pools[S.KIND_CONST]), cat(pools[S.KIND_RANK1])
    lev_d, leaf_d, xd = torch.from_numpy(host).to(dev), torch.from_numpy(leaf).to(dev), x.to(dev)
    lm, cd, lp = _Guarded(B * P * Cmax, dev), _Guarded(B * P * Cmax, dev), _Guarded(B * P, dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    capi.call("ck_squared_path_steps", ptr(full_d), ptr(cst_d), ptr(rk_d), host.ctypes.data, lev_d.data_ptr(), L_max * W, S_max,
              leaf.ctypes.data, leaf_d.data_ptr(), 0, P, xd.data_ptr(), D, None, lm.out.data_ptr(), P * Cmax, Cmax, cd.out.data_ptr(),
              P * Cmax, Cmax, lp.out.data_ptr(), P, 1, Cmax, B, R_rows, 1 if cplx else 0, _stream(dev))
    torch.cuda.synchronize(dev)
    got_m, got_c, got_p = lm.read().reshape(B, P, Cmax), cd.read().reshape(B, P, Cmax), lp.read().reshape(B, P)
    for si, ((_, want, _, _), shape) in enumerate(zip(cases, shapes)):
        C = Cs[si]
        assert bool((got_m[:, si, C:] == -np.inf).all()) and bool((got_c[:, si, C:] == -np.inf).all()), shape
        w = want[:, :C]
        live = torch.isfinite(w).any(dim=1)
        gm = got_m[:, si, :C].double()
        assert not bool(torch.isnan(gm).any()) and bool((gm[~live] == -np.inf).all())
        _held(gm[live], w[live], torch.ones_like(w[live], dtype=torch.bool), f"{shape}: log m")
        wc = w[live] - torch.logsumexp(w[live], dim=1, keepdim=True)
        _held(got_c[live][:, si, :C], wc, torch.ones_like(wc, dtype=torch.bool), f"{shape}: conditionals", 2.0)
        assert bool(torch.isnan(got_c[~live][:, si, :C]).all()) and bool(torch.isnan(got_p[~live][:, si]).all())
        own = x[:, si + 1]
        assert torch.equal(got_p[live][:, si], got_c[live][:, si].gather(1, own[live][:, None])[:, 0])


# ---- 6. the codec ---------------------------------------------------------------------------------------------------------------
def test_compress_and_decompress(hip_device):
    """3 rows of the 4 x 4 Categorical circuit: `decompress` gives the rows back, the stepwise blobs (16 one-step calls) are those
    of the all-steps call, and a blob is no longer than the quantised ideal plus `codec.OVERHEAD_BITS`."""
    from cirkit_amd import codec

    sq = _cat_circuit(str(hip_device))
    x = A.cat_rows()
    blobs, counts = codec.compress(sq, x, return_counts=True)
    batched = codec.compress(sq, x.to(hip_device), batched=True)
    assert blobs == batched
    back = codec.decompress(sq, blobs)
    assert back.dtype == torch.int64 and torch.equal(back, x)
    bits = np.asarray([8 * len(b) for b in blobs])
    ideal = codec.ideal_bits(counts, 16)
    print(f"coded {bits.tolist()} bits, quantised ideal {np.round(ideal, 1).tolist()}")
    assert bool((bits <= ideal + codec.OVERHEAD_BITS).all())
    raster = list(range(16))
    assert torch.equal(codec.decompress(sq, codec.compress(sq, x, raster, precision=12), raster, precision=12), x)
    gone = x.clone()
    gone[1, 3] = -1
    with pytest.raises(ValueError, match="missing"):
        codec.compress(sq, gone)
    with pytest.raises(ValueError):
        codec.compress(sq, x, precision=9)  # (256 states need 10 bits)
    with pytest.raises(ValueError, match="permutation"):
        codec.compress(sq, x, list(range(15)))


# ---- 7. edge rows and refusals --------------------------------------------------------------------------------------------------
def test_edge_rows(hip_device):
    sq = _emb32_circuit(str(hip_device))
    from cirkit_amd.squared_sampling import tree_order

    order = tree_order(sq.plan)
    xd = torch.from_numpy(S.golden()["emb32_x"])[:5].to(hip_device)
    cond, lp, tab = sq.autoregressive_conditionals(xd).clone(), sq.autoregressive_log_probs(xd).clone(), sq.coding_tables(xd).clone()
    bad = xd.clone()
    bad[1, order[2]] = -1
    bad[3, order[9]] = 3  # (3 states: 0 .. 2)
    good = [0, 2, 4]
    c2, l2, t2 = sq.autoregressive_conditionals(bad), sq.autoregressive_log_probs(bad), sq.coding_tables(bad)
    assert bool(torch.isnan(c2[[1, 3]]).all()) and bool(torch.isnan(l2[[1, 3]]).all())
    assert torch.equal(c2[good], cond[good]) and torch.equal(l2[good], lp[good]) and torch.equal(t2[good], tab[good])
    T = 1 << 16
    flat = torch.tensor([0, T // 3 + T - (T // 3) * 3, 2 * (T // 3) + T - (T // 3) * 3, T], dtype=torch.int32)
    assert bool((t2[[1, 3]].cpu() == flat).all())
    # what a decoder holds at step 2: nothing from there on -- those entries are not read
    held = xd.clone()
    held[:, order[2:]] = -1
    assert torch.equal(sq.autoregressive_conditionals(held, positions=[0, 2]), cond[:, [0, 2]])
    assert bool(torch.isnan(sq.autoregressive_log_probs(held, positions=[2])).all())  # (the log probability reads the step's own entry)
    assert torch.equal(sq.autoregressive_conditionals(xd), cond)  # a later valid call is unaffected


def test_a_prefix_without_mass(hip_device):
    """State 1 of variable 0 of the tiny circuit made impossible (every unit 0 there): its conditional is -inf at that state, and
    a row that holds it has no mass from the next step on: NaN there, nothing faults, the other rows are finite."""
    from cirkit_amd.squared import HipSquaredCircuit
    from cirkit_amd.squared_sampling import tree_order

    plan, tensors, states = R.tiny_case("cp")
    tensors = {k: np.array(v, copy=True) for k, v in tensors.items()}
    hit = 0
    for l in plan.layers:
        if l.inputs is None:
            names = [n.config["tensor"] for g in l.params.values() for n in g.nodes if n.op == "tensor"]
            for f in np.nonzero(np.asarray(l.scope_idx)[:, 0] == 0)[0]:
                tensors[names[0]][f, :, 1] = 0.0  # (F, K, states)
                hit += 1
    assert hit == 1
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    order = tree_order(sq.plan)
    i0 = order.index(0)
    x = A.tiny_rows().clone()
    x[:, 0] = torch.tensor([0, 1, 2, 1, 0])
    cond = sq.autoregressive_conditionals(x.to(hip_device)).cpu()
    lp = sq.autoregressive_log_probs(x.to(hip_device)).cpu()
    dead = x[:, 0] == 1
    assert bool((cond[:, i0, 1] == -np.inf).all()) and bool(torch.isfinite(cond[:, i0, [0, 2]]).all())
    assert bool((lp[dead, i0] == -np.inf).all())
    assert bool(torch.isnan(cond[dead][:, i0 + 1:]).all()) and bool(torch.isnan(lp[dead][:, i0 + 1:]).all())
    assert bool(torch.isfinite(cond[~dead]).logical_or(cond[~dead] == -np.inf).all()) and bool(torch.isfinite(lp[~dead]).all())
    tab = sq.coding_tables(x.to(hip_device)).cpu()
    assert bool((tab[..., 0] == 0).all()) and bool((tab[..., -1] == 1 << 16).all()) and bool((torch.diff(tab, dim=2) >= 1).all())


def test_refusals(hip_device):
    from cirkit_amd import codec
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.squared import HipSquaredCircuit
    from cirkit_amd.squared_sampling import path_plan
    from cirkit_amd.templates import InputSpec, build_plan, quad_graph

    plan, tensors, x = R.gauss_case()
    gs = HipSquaredCircuit(plan, tensors, device=hip_device)
    xg = x[:2].to(torch.float32).to(hip_device)
    before = torch.cuda.memory_allocated(hip_device)
    for call in (lambda: gs.autoregressive_conditionals(xg), lambda: gs.autoregressive_log_probs(xg), lambda: gs.coding_tables(xg),
                 lambda: codec.compress(gs, np.zeros((2, plan.num_variables), dtype=np.int64)), lambda: codec.decompress(gs, [b"\0" * 8])):
        with pytest.raises(NotImplementedError, match="Gaussian"):
            call()
    assert torch.cuda.memory_allocated(hip_device) == before
    dag = build_plan(quad_graph(4, 4), input_layer=InputSpec("embedding", 3), sum_product="cp", num_input_units=4, num_sum_units=4,
                     sum_activation="none", semiring="complex-lse-sum")
    with pytest.raises(NotImplementedError):  # (a QuadGraph is refused by the constructor, and its ancestries are no paths)
        HipSquaredCircuit(dag, init_plan_tensors(dag, seed=3), device=hip_device)
    with pytest.raises(NotImplementedError, match="DAG"):
        path_plan(dag, 5)
    sq = _emb32_circuit(str(hip_device))
    xd = torch.from_numpy(S.golden()["emb32_x"])[:4].to(hip_device)
    for order in (list(range(15)), [0] * 16, list(range(1, 17))):
        with pytest.raises(ValueError, match="permutation"):
            sq.autoregressive_conditionals(xd, order)
    with pytest.raises(ValueError, match="permutation"):
        sq.autoregressive_log_probs(xd, list(range(16)), integrate_vars=[3])  # (an integrated variable in the order)
    with pytest.raises(ValueError):
        sq.autoregressive_conditionals(xd, integrate_vars=list(range(16)))
    for positions in ([16], [-1], [], torch.zeros(16, dtype=torch.bool)):
        with pytest.raises(ValueError):
            sq.coding_tables(xd, positions=positions)
    for precision in (7, 25, 16.5):
        with pytest.raises(ValueError):
            sq.coding_tables(xd, precision=precision)
    with pytest.raises(ValueError):
        sq.autoregressive_conditionals(xd[:, :15])
    with pytest.raises(ValueError):
        sq.autoregressive_conditionals(xd, rows_per_chunk=0)
    assert sq.autoregressive_conditionals(xd, integrate_vars=[3]).shape == (4, 15, 3)
