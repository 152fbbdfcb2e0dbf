"""The parameter prologue entry by entry: `ck_param_softmax_batch` (kinds 0, 1, 2, 4, 5, job lists, refusals) and the per-node
kernels `ck_param_softmax`, `ck_param_transpose_last2(_c)`, `ck_param_table_integral_row`, `ck_param_binomial_table`
(cirkit_amd/csrc/ck_param.hip) against the fp64 restatement of tests/prologue_restatement.py, on both sides of every shape
boundary of the kernels, and the host guards that decide which jobs are registered.

Memory.  Every output lives inside a larger buffer pre-filled with a NaN bit pattern no kernel produces, `GUARD` words before
and after it: the guards must be untouched and every word the kernel owns written (`_Guarded.read`).

Tolerance (the convention of tests/test_posterior_marginals.py).  The yardstick of a case is the error of the SAME restatement
run in fp32 by torch on the CPU against its fp64 run, on the case's own inputs; the GPU must be within 4 x that, with a floor
of 1e-6.  Linear outputs: error relative to max|row|; log outputs: absolute.  Nothing in a bar comes from what the GPU returns.
Every case prints `PROLOGUE <kind> <case> err yard ratio` (ratio = err / max(yard, floor / 4): a case passes iff ratio <= 4);
the worst per kind are in LAB_NOTES.md, "Parameter prologue".

Where the log-table is -inf.  The reference layer takes the log of an fp32 softmax (layers/input.py:405-408), which is -inf once
exp(theta - max) underflows, below log(2^-149) = -103.28; the kind-1 kernels write -inf where theta - max < -103.9 and the
restatement (log_softmax) stays finite.  So a log entry whose reference value is below `LOG_CUT` = -103 may be -inf or within
the bar, an entry above it must be finite and within the bar, and a reference -inf must be exactly -inf.  Kinds 4 / 5 sum such
entries with weights <= 1: what the cut drops is at most e^-103.9 in total, 6e-9 of a result above `DENSE_CUT` = -85, so
results above -85 are compared and those below only required not to be NaN (kind 5: also relative to the row's scale, below
which fp32 `out` underflows)."""
import pytest
import torch

from guarded_buffers import GUARD, NAN_BITS, NEG_INF, _Guarded, _logits, _stream  # noqa: F401
from prologue_restatement import (binomial_table, integral_row, log_table, softmax_rows, table_dense, to_tiled,
                                  transpose_last2)

pytestmark = pytest.mark.gpu

FLOOR = 1e-6
LOG_CUT = -103.0
DENSE_CUT = -85.0
FAMILIES = ["normal", "shift+", "shift-", "spread", "const", "neginf"]
WORST: dict[str, tuple] = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for kind in sorted(WORST):
        r, case, err, yard = WORST[kind]
        print(f"\nPROLOGUE-WORST {kind}: ratio {r:.3f} (err {err:.3e}, yardstick {yard:.3e}) at {case}")


def _report(kind, case, err, yard):
    err, yard = float(err), float(yard)
    ratio = err / max(yard, FLOOR / 4)
    print(f"PROLOGUE {kind} {case} err {err:.3e} yard {yard:.3e} ratio {ratio:.3f}")
    if kind not in WORST or ratio > WORST[kind][0]:
        WORST[kind] = (ratio, case, err, yard)
    assert err <= max(4 * yard, FLOOR), f"{kind} {case}: error {err:.3e} above 4 x the fp32 yardstick {yard:.3e} (floor {FLOOR})"


def _check_linear(kind, case, got, x):
    """got (rows, len) = softmax(x) in linear space: error relative to max|row|, exact zeros at -inf logits, rows summing to 1,
    the largest logit keeping the largest probability."""
    got = got.double()
    ref, yard = softmax_rows(x.double()), softmax_rows(x).double()
    assert bool(torch.isfinite(got).all()) and bool((got >= 0).all())
    dead = torch.isinf(x)
    assert bool((got[dead] == 0).all()), "an entry with a -inf logit is not exactly 0"
    scale = ref.abs().amax(dim=-1, keepdim=True)
    err, y = ((got - ref).abs() / scale).max(), ((yard - ref).abs() / scale).max()
    top = x.argmax(dim=-1, keepdim=True)
    assert bool((got.gather(-1, top) == got.amax(dim=-1, keepdim=True)).all()), "argmax not preserved"
    sum_err, sum_y = (got.sum(-1) - 1).abs().max(), (yard.sum(-1) - 1).abs().max()
    assert float(sum_err) <= max(4 * max(float(y), float(sum_y)), FLOOR), (kind, case, float(sum_err), float(sum_y))
    _report(kind, case, err, y)


def _check_log(kind, case, got, ref, yard, cut=LOG_CUT, below_is_free=False):
    """got = log-space output against ref (fp64) with yardstick run `yard` (fp32): see the module docstring."""
    got, yard = got.double(), yard.double()
    assert not bool(torch.isnan(got).any()), "NaN in a log output"
    ninf = torch.isinf(ref)
    assert bool((got[ninf] == NEG_INF).all()), "a reference -inf is not exactly -inf"
    live = ~ninf & (ref > cut)
    assert bool(torch.isfinite(got[live]).all()), "a log entry above the cut is not finite"
    err = (got[live] - ref[live]).abs().max() if bool(live.any()) else torch.tensor(0.0)
    y = (yard[live] - ref[live]).abs().max() if bool(live.any()) else torch.tensor(0.0)
    low = ~ninf & ~live
    if bool(low.any()) and not below_is_free:
        ok = (got[low] == NEG_INF) | ((got[low] - ref[low]).abs() <= max(4 * float(y), FLOOR))
        assert bool(ok.all()), "an entry below the cut is neither -inf nor within the bar"
    _report(kind, case, err, y)


def _job(inp, out, rows, ln, k, kind, in2=None, idx=None, out2=None):
    return (inp.data_ptr(), out.data_ptr(), int(rows), int(ln), int(k), int(kind), None if in2 is None else in2.data_ptr(),
            None if idx is None else idx.data_ptr(), None if out2 is None else out2.data_ptr())


def _launch(jobs, dev, block_begin=0):
    """`ck_param_softmax_batch` on a raw job array (block_begin is documented as ignored on input)."""
    from cirkit_amd import _capi as capi

    arr = (capi.SoftmaxJob * len(jobs))()
    for n, (a, (i, o, rows, ln, k, kind, in2, idx, out2)) in enumerate(zip(arr, jobs)):
        a.inp, a.out, a.rows, a.len, a.k, a.kind = i, o, rows, ln, k, kind
        a.block_begin = block_begin if block_begin == 0 else block_begin * (n + 1) * (-1) ** n
        a.in2, a.idx, a.out2 = in2, idx, out2
    capi.call("ck_param_softmax_batch", arr, len(jobs), _stream(dev))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ kind 0
KIND0_LENS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 516, 1024, 1028, 2048, 4096, 4100, 5000]
KIND0_ROWS = [1, 3, 63, 64, 65, 130]


@pytest.mark.parametrize("ln", KIND0_LENS)
def test_kind0_rows(hip_device, ln):
    """Every (rows, value family) pair of a row length as one job each of a `ParamBatch` (36 jobs, each with its own guarded
    output): len <= 32 (two rows per wave), 33..64 / 65..128 / 129..256 (rows in registers), the generic loop, and the long-row
    kernel (512..4096, len % 4 == 0: N4 = 2, 4, 8, 16 at 512 / 1024 / 2048 / 4096; 516 and 1028 cross into the next one)."""
    from cirkit_amd.parameters import ParamBatch

    g = torch.Generator().manual_seed(1000 + ln)
    pb, cases = ParamBatch(), []
    for rows in KIND0_ROWS:
        for fam in FAMILIES:
            x = _logits((rows, ln), fam, g)
            xd, o = x.to(hip_device), _Guarded(rows * ln, hip_device)
            pb.add_softmax(xd, o.out.view(rows, ln))
            cases.append((rows, fam, x, o))
    pb.launch(_stream(hip_device))
    torch.cuda.synchronize()
    for rows, fam, x, o in cases:
        _check_linear("kind0", f"len={ln} rows={rows} {fam}", o.read().view(rows, ln), x)


def test_kind0_long_rows_grid_stride(hip_device):
    """More than 16384 long rows: the grid is capped at 4096 workgroups of 4 rows and strides."""
    rows, ln = 16384 + 37, 512
    x = _logits((rows, ln), "normal", torch.Generator().manual_seed(7))
    x[-1, 5] = NEG_INF
    xd, o = x.to(hip_device), _Guarded(rows * ln, hip_device)
    _launch([_job(xd, o.out, rows, ln, 0, 0)], hip_device)
    _check_linear("kind0", f"len={ln} rows={rows} grid-stride", o.read().view(rows, ln), x)


def test_kind0_misaligned_source_takes_the_generic_path(hip_device):
    """len = 512 from a source 4 bytes off 16-byte alignment: not a long-row job (16-byte loads), same values."""
    rows, ln = 67, 512
    x = _logits((rows, ln), "normal", torch.Generator().manual_seed(8))
    buf = torch.zeros(rows * ln + 8, device=hip_device)
    src = buf[1:1 + rows * ln]
    src.copy_(x.reshape(-1))
    assert src.data_ptr() % 16 == 4
    o, o2 = _Guarded(rows * ln, hip_device), _Guarded(rows * ln, hip_device)
    _launch([_job(src, o.out, rows, ln, 0, 0)], hip_device)
    got = o.read().view(rows, ln)
    _check_linear("kind0", f"len={ln} rows={rows} source+4B", got, x)
    xa = x.to(hip_device)
    _launch([_job(xa, o2.out, rows, ln, 0, 0)], hip_device)  # (the aligned source: the long-row kernel)
    long = o2.read().view(rows, ln).double()
    yard = (softmax_rows(x).double() - softmax_rows(x.double())).abs().max() / softmax_rows(x.double()).amax()
    assert float((got.double() - long).abs().max() / long.amax()) <= 2 * max(4 * float(yard), FLOOR)


def test_long_row_output_4_bytes_off_alignment(hip_device):
    """... and an OUTPUT 4 bytes off: the generic path again, nothing outside the rows written."""
    rows, ln = 5, 1024
    x = _logits((rows, ln), "normal", torch.Generator().manual_seed(9))
    o = _Guarded(rows * ln, hip_device, lead=1)
    assert o.out.data_ptr() % 16 == 4
    _launch([_job(x.to(hip_device), o.out, rows, ln, 0, 0)], hip_device)
    _check_linear("kind0", f"len={ln} rows={rows} output+4B", o.read().view(rows, ln), x)


# ------------------------------------------------------------------------------------------------------------ kind 2
@pytest.mark.parametrize("rows", [32, 96])
def test_kind2_tiled_layout(hip_device, rows):
    from cirkit_amd.parameters import ParamBatch

    g = torch.Generator().manual_seed(rows)
    for fam in FAMILIES:
        x = _logits((rows, 32), fam, g)
        xd, o = x.to(hip_device), _Guarded(rows * 32, hip_device)
        pb = ParamBatch()
        pb.add_softmax(xd.view(rows // 32, 32, 32), o.out.view(rows // 32, 32, 32), layout=1)
        pb.launch(_stream(hip_device))
        torch.cuda.synchronize()
        got = o.read().view(rows // 32, 1024)
        # un-tile with the documented permutation, then the same checks as kind 0
        ident = to_tiled(torch.arange(1024.0).view(1, 32, 32))[0].long()  # tiled position -> row-major index
        rowmajor = torch.empty_like(got)
        rowmajor[:, ident] = got
        _check_linear("kind2", f"rows={rows} {fam}", rowmajor.view(rows, 32), x)
        want = to_tiled(softmax_rows(x.double()).view(rows // 32, 32, 32))
        assert float((got.double() - want).abs().max()) <= 1e-5  # (every value in ITS place: a swap moves entries by ~1/32)


def test_kind2_consumer_reads_what_kind0_gives(hip_device):
    """One 32-unit sum layer on the tiled weights (CK_W_TILED_F32) and on the row-major ones: bit-identical outputs."""
    from cirkit_amd import _capi as capi

    F, B = 3, 70
    g = torch.Generator().manual_seed(21)
    theta = torch.randn(F, 32, 32, generator=g).to(hip_device)
    x = (torch.randn(F, 1, B, 32, generator=g) * 3 - 4).to(hip_device)
    w_row, w_tiled = _Guarded(F * 1024, hip_device), _Guarded(F * 1024, hip_device)
    _launch([_job(theta, w_row.out, F * 32, 32, 0, 0), _job(theta, w_tiled.out, F * 32, 32, 0, 2)], hip_device)
    w_row.read(), w_tiled.read()
    row_off = (torch.arange(F, dtype=torch.int64) * (B * 32)).reshape(F, 1).to(hip_device)
    outs = []
    for w, layout in ((w_row, capi.CK_W_ROWMAJOR), (w_tiled, capi.CK_W_TILED_F32)):
        o = _Guarded(F * B * 32, hip_device)
        capi.call("ck_sum_lse_fwd", x.data_ptr(), row_off.data_ptr(), w.out.data_ptr(), o.out.data_ptr(), F, 1, B, 32, 32,
                  capi.CK_SUM_CAT, layout, _stream(hip_device))
        torch.cuda.synchronize()
        o.read()
        outs.append(o.raw())
    assert torch.equal(outs[0], outs[1])
    want = torch.logsumexp(x.cpu().double()[:, 0, :, None, :] + torch.log_softmax(theta.cpu().double(), -1)[:, None], dim=-1)
    assert float((outs[0].view(torch.float32).view(F, B, 32).double() - want).abs().max()) <= 1e-4


# ------------------------------------------------------------------------------------------------------------ kind 1
KIND1_K = [1, 5, 31, 32, 33, 64, 100]
KIND1_C = [1, 2, 3, 4, 10, 252, 255, 256, 257, 260, 300]


@pytest.mark.parametrize("C", KIND1_C)
@pytest.mark.parametrize("K", KIND1_K)
def test_kind1_log_table(hip_device, K, C):
    """(F, K, C) -> (F, C + 1, K): the rows-in-registers form (C <= 256, C % 4 == 0) and the LDS form, units walked with
    the `min(k0 + ..., K - 1)` clamps (K % 4 != 0, K < 4, K not a multiple of the 32 units of a pass), F in {1, 3}."""
    from cirkit_amd.parameters import ParamBatch

    g = torch.Generator().manual_seed(K * 1000 + C)
    pb, cases = ParamBatch(), []
    for F in (1, 3):
        for fam in FAMILIES:
            th = _logits((F, K, C), fam, g)
            o = _Guarded(F * (C + 1) * K, hip_device)
            pb.add_log_table(th.to(hip_device), o.out.view(F, C + 1, K))
            cases.append((F, fam, th, o))
    pb.launch(_stream(hip_device))
    torch.cuda.synchronize()
    for F, fam, th, o in cases:
        got = o.read().view(F, C + 1, K)
        assert bool((got[:, C] == 0).all()), "the integral row is not exactly 0"
        _check_log("kind1", f"K={K} C={C} F={F} {fam}", got, log_table(th.double()), log_table(th))


# ------------------------------------------------------------------------------------------------------- kinds 4 and 5
DENSE_C = [1, 4, 10, 31, 32, 33, 255, 256, 260, 300]


def _dense_case(dev, kind, K, C, fam, with_idx, g):
    F = 3
    idx = [2, 0, 2, 1, 0] if with_idx else None
    Fd = len(idx) if with_idx else F
    th = _logits((F, K, C), fam, g)
    dense = _logits((Fd, K, K), "neginf" if fam == "neginf" else ("const" if fam == "const" else "normal"), g)
    o = _Guarded(Fd * (C + 1) * K, dev)
    o2 = _Guarded(Fd * (C + 1), dev) if kind == 5 else None
    idx_d = None if idx is None else torch.tensor(idx, dtype=torch.int64, device=dev)
    keep = (th.to(dev), dense.to(dev), idx_d)
    return dict(F=F, Fd=Fd, th=th, dense=dense, idx=idx, o=o, o2=o2, keep=keep, fam=fam, kind=kind, K=K, C=C)


def _dense_check(c):
    Fd, C, K = c["Fd"], c["C"], c["K"]
    ref = table_dense(c["th"].double(), c["dense"].double(), c["idx"])
    yard = table_dense(c["th"], c["dense"], c["idx"])
    case = f"K={K} C={C} idx={'map' if c['idx'] else 'none'} {c['fam']}"
    got = c["o"].read().view(Fd, C + 1, K)
    if c["kind"] == 4:
        _check_log("kind4" if K == 32 else "kind4-wide", case, got, ref, yard, cut=DENSE_CUT, below_is_free=True)
        return
    scale = c["o2"].read().view(Fd, C + 1).double()
    assert bool(torch.isfinite(got).all()) and bool((got >= 0).all()), "kind 5: out must be finite and >= 0"
    assert bool(torch.isfinite(scale).all()), "kind 5: out2 must be finite"
    v = torch.log(got.double()) + scale[..., None]
    # ... wherever the reference is above the fp32 underflow of its row (and above the cut of the table)
    reach = (ref - ref.amax(dim=-1, keepdim=True)) > DENSE_CUT
    v = torch.where(reach, v, ref)
    _check_log("kind5", case, v, ref, yard, cut=DENSE_CUT, below_is_free=True)


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("C", DENSE_C)
@pytest.mark.parametrize("kind,K", [(4, 32), (4, 64), (5, 32)])
def test_kind4_kind5_dense_on_table(hip_device, kind, K, C, with_idx):
    """The dense layer applied to the table: rows form (C <= 256, C % 4 == 0), general form, and the 64-unit WIDE launch;
    idx None, and a map with repeats and Fd != F."""
    from cirkit_amd.parameters import ParamBatch

    g = torch.Generator().manual_seed(kind * 100000 + K * 1000 + C + (7 if with_idx else 0))
    pb, cases = ParamBatch(), []
    for fam in FAMILIES:
        c = _dense_case(hip_device, kind, K, C, fam, with_idx, g)
        thd, dd, idx_d = c["keep"]
        pb.add_log_table_dense(thd, dd, idx_d, c["o"].out.view(c["Fd"], C + 1, K), None if kind == 4 else c["o2"].out.view(c["Fd"], C + 1))
        cases.append(c)
    pb.launch(_stream(hip_device))
    torch.cuda.synchronize()
    for c in cases:
        _dense_check(c)


# ------------------------------------------------------------------------------------------------------------ job lists
def _mixed_jobs(dev, n, g):
    """n small jobs of all kinds interleaved -- short, medium, generic and long rows, tiled rows, both table forms, both dense
    forms at 32 units, both at 64 (the WIDE pass), kind 5 -- each with its own inputs and guarded outputs."""
    makers = [
        lambda: ("r", 0, 5, 7), lambda: ("t", 1, 5, 8), lambda: ("d", 4, 32, 8), lambda: ("r", 0, 6, 512),
        lambda: ("d", 4, 64, 12), lambda: ("r", 0, 9, 100), lambda: ("t", 1, 33, 10), lambda: ("d", 5, 32, 10),
        lambda: ("r", 2, 64, 32), lambda: ("d", 4, 64, 10), lambda: ("r", 0, 70, 300), lambda: ("d", 4, 32, 10),
        lambda: ("r", 0, 3, 1024), lambda: ("d", 5, 32, 8), lambda: ("r", 0, 17, 40),
    ]
    jobs = []
    for i in range(n):
        what, kind, a, b = makers[i % len(makers)]()
        if what == "r":
            rows, ln = a, b
            x = _logits((rows, ln), "normal", g).to(dev)
            jobs.append(dict(keep=[x], outs=lambda rows=rows, ln=ln: [_Guarded(rows * ln, dev)],
                             job=lambda o, x=x, rows=rows, ln=ln, kind=kind: _job(x, o[0].out, rows, ln, 0, kind)))
        elif what == "t":
            K, C, F = a, b, 2
            x = _logits((F, K, C), "normal", g).to(dev)
            jobs.append(dict(keep=[x], outs=lambda K=K, C=C, F=F: [_Guarded(F * (C + 1) * K, dev)],
                             job=lambda o, x=x, K=K, C=C, F=F: _job(x, o[0].out, F, C, K, 1)))
        else:
            K, C, F = a, b, 2
            x, w = _logits((F, K, C), "normal", g).to(dev), _logits((3, K, K), "normal", g).to(dev)
            idx = torch.tensor([1, 0, 1], dtype=torch.int64, device=dev)
            jobs.append(dict(keep=[x, w, idx],
                             outs=lambda K=K, C=C, kind=kind: [_Guarded(3 * (C + 1) * K, dev)] + ([_Guarded(3 * (C + 1), dev)] if kind == 5 else []),
                             job=lambda o, x=x, w=w, idx=idx, K=K, C=C, kind=kind: _job(x, o[0].out, 3, C, K, kind, w, idx,
                                                                                        o[1].out if kind == 5 else None)))
    return jobs


@pytest.mark.parametrize("n", [1, 48, 49, 110])
def test_job_lists_equal_single_launches(hip_device, n):
    """Lists of 1, 48 (= kMaxJobs), 49 and 110 mixed jobs -- cut into several launches, wide and narrow jobs in two passes,
    long rows in launches of their own -- with zero and with garbage `block_begin`: every job's output bit-identical to the
    job launched alone."""
    specs = _mixed_jobs(hip_device, n, torch.Generator().manual_seed(n))
    alone = []
    for s in specs:
        o = s["outs"]()
        _launch([s["job"](o)], hip_device)
        alone.append([b.read().view(torch.int32).clone() for b in o])
    for garbage in (0, 12345):
        outs = [s["outs"]() for s in specs]
        _launch([s["job"](o) for s, o in zip(specs, outs)], hip_device, block_begin=garbage)
        for i, (o, a) in enumerate(zip(outs, alone)):
            for b, want in zip(o, a):
                assert torch.equal(b.read().view(torch.int32), want), f"job {i} of {n} (block_begin {garbage}) differs from its single launch"


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_before_any_launch(hip_device):
    """Host-side checks of single-job lists: the error `capi.call` raises, and that nothing was written."""
    dev = hip_device
    x = torch.zeros(64 * 700, device=dev)
    w = torch.zeros(64 * 64, device=dev)
    o, o2 = _Guarded(64 * 701, dev), _Guarded(701, dev)
    cases = [
        ("kind 3", _job(x, o.out, 32, 32, 0, 3), ValueError, "unknown kind"),
        ("kind 6", _job(x, o.out, 32, 32, 0, 6), ValueError, "unknown kind"),
        ("kind 2, len 31", _job(x, o.out, 32, 31, 0, 2), ValueError, "len = 32"),
        ("kind 2, rows 33", _job(x, o.out, 33, 32, 0, 2), ValueError, "rows % 32"),
        ("kind 4, K 48", _job(x, o.out, 1, 8, 48, 4, w), ValueError, "k = 32"),
        ("kind 4, no in2", _job(x, o.out, 1, 8, 32, 4), ValueError, "in2"),
        ("kind 5, K 64", _job(x, o.out, 1, 8, 64, 5, w, None, o2.out), ValueError, "k = 32"),
        ("kind 5, no out2", _job(x, o.out, 1, 8, 32, 5, w), ValueError, "out2"),
        ("kind 1, K 0", _job(x, o.out, 1, 8, 0, 1), ValueError, "k > 0"),
        ("kind 1, LDS", _job(x, o.out, 1, 316, 128, 1), NotImplementedError, "too large"),
        ("kind 1, LDS (transposed tile)", _job(x, o.out, 1, 641, 63, 1), NotImplementedError, "too large"),
        ("kind 4, LDS", _job(x, o.out, 1, 571, 64, 4, w), NotImplementedError, "too large"),
        ("kind 5, LDS", _job(x, o.out, 1, 1243, 32, 5, w, None, o2.out), NotImplementedError, "too large"),
    ]
    for name, job, exc, text in cases:
        with pytest.raises(exc, match=text):
            _launch([job], dev)
    torch.cuda.synchronize()
    assert bool((o.raw() == NAN_BITS).all()) and bool((o2.raw() == NAN_BITS).all()), "a refused job wrote something"
    from cirkit_amd import _capi as capi

    with pytest.raises(ValueError, match="no jobs"):
        capi.call("ck_param_softmax_batch", None, 0, _stream(dev))


# ------------------------------------------------------------------------------------------------------------ per node
@pytest.mark.parametrize("log_space", [0, 1])
@pytest.mark.parametrize("inner", [1, 5])
def test_param_softmax_node(hip_device, inner, log_space):
    """`ck_param_softmax` over the middle axis of (outer, len, inner): one wave per line (inner = 1), one thread per line."""
    from cirkit_amd import _capi as capi

    g = torch.Generator().manual_seed(inner * 2 + log_space)
    lens = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 512, 1028] if inner == 1 else [1, 2, 33, 64, 65, 257]
    for ln in lens:
        for outer in (1, 3, 65):
            for fam in FAMILIES:
                x = _logits((outer, inner, ln), fam, g)  # (softmax axis last for `_logits`)
                xin = x.transpose(1, 2).contiguous()  # (outer, len, inner) as the kernel sees it
                o = _Guarded(outer * ln * inner, hip_device)
                capi.call("ck_param_softmax", xin.to(hip_device).data_ptr(), o.out.data_ptr(), outer, ln, inner, log_space, _stream(hip_device))
                torch.cuda.synchronize()
                got = o.read().view(outer, ln, inner).transpose(1, 2)
                case = f"inner={inner} len={ln} outer={outer} {fam}"
                if log_space:
                    _check_log("softmax-node-log", case, got, softmax_rows(x.double(), True), softmax_rows(x, True), cut=-1e30)
                else:
                    _check_linear("softmax-node", case, got.reshape(-1, ln), x.reshape(-1, ln))


TR = [1, 31, 32, 33, 70]


@pytest.mark.parametrize("Bd", TR)
@pytest.mark.parametrize("A", TR)
def test_transpose_last2(hip_device, A, Bd):
    """(R, A, Bd) -> (R, out_rows, A): float with and without the log (an entry equal to 0 gives exactly -inf), complex;
    out_rows in {Bd, Bd + 1}: rows Bd .. out_rows - 1 of every block stay untouched."""
    from cirkit_amd import _capi as capi

    R = 3
    g = torch.Generator().manual_seed(A * 100 + Bd)
    for extra in (0, 1):
        rows = Bd + extra
        owned = torch.zeros(R, rows, A, dtype=torch.bool)
        owned[:, :Bd] = True
        for take_log in (0, 1):
            x = torch.rand(R, A, Bd, generator=g) + 0.01
            if take_log:
                x[0, 0, 0] = 0.0
                x[R - 1, A - 1, Bd - 1] = 0.0
            o = _Guarded(R * rows * A, hip_device)
            capi.call("ck_param_transpose_last2", x.to(hip_device).data_ptr(), o.out.data_ptr(), R, A, Bd, take_log, rows, _stream(hip_device))
            torch.cuda.synchronize()
            got = o.read(owned).view(R, rows, A)[:, :Bd]
            if take_log:
                assert got[0, 0, 0] == NEG_INF and got[R - 1, Bd - 1, A - 1] == NEG_INF
                _check_log("transpose-log", f"A={A} Bd={Bd} out_rows={rows}", got, transpose_last2(x.double(), True), transpose_last2(x, True), cut=-1e30)
            else:
                assert torch.equal(got, transpose_last2(x))
        xc = torch.complex(torch.randn(R, A, Bd, generator=g), torch.randn(R, A, Bd, generator=g))
        o = _Guarded(R * rows * A * 2, hip_device)
        capi.call("ck_param_transpose_last2_c", torch.view_as_real(xc).contiguous().to(hip_device).data_ptr(), o.out.data_ptr(), R, A, Bd, rows,
                  _stream(hip_device))
        torch.cuda.synchronize()
        got = o.read(owned[..., None].expand(R, rows, A, 2).contiguous()).view(R, rows, A, 2)[:, :Bd]
        assert torch.equal(torch.view_as_complex(got.contiguous()), transpose_last2(xc))


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_table_integral_row(hip_device, mode):
    g = torch.Generator().manual_seed(mode)
    for F, C, K in [(1, 1, 1), (3, 5, 32), (2, 300, 33), (2, 7, 300), (1, 256, 64)]:
        if mode == 3:
            K = 2 * K  # K floats = K / 2 complex pairs
        for fam in (FAMILIES if mode == 1 else ["normal"]):
            rows = _logits((F, K, C), fam, g).transpose(1, 2).contiguous()  # (F, C, K), logsumexp over C
            o = _Guarded(F * (C + 1) * K, hip_device)
            o.out.view(F, C + 1, K)[:, :C].copy_(rows)
            from cirkit_amd import _capi as capi

            capi.call("ck_param_table_integral_row", o.out.data_ptr(), F, C, K, mode, _stream(hip_device))
            torch.cuda.synchronize()
            got = o.read().view(F, C + 1, K)
            assert torch.equal(got[:, :C].view(torch.int32), rows.view(torch.int32)), "the rows of the table were changed"
            table64 = torch.cat([rows.double(), torch.zeros(F, 1, K, dtype=torch.float64)], dim=1)
            ref = integral_row(table64, mode)
            if mode == 1:
                _check_log("integral-row", f"F={F} C={C} K={K} {fam}", got[:, C], ref, integral_row(table64.float(), 1), cut=-1e30)
            else:
                assert torch.equal(got[:, C].double(), ref)


@pytest.mark.parametrize("is_logits", [0, 1])
@pytest.mark.parametrize("total_count", [0, 1, 255])
def test_binomial_table(hip_device, total_count, is_logits):
    """`ck_param_binomial_table` against torch.distributions.Binomial.log_prob in fp64; the fp32 yardstick is the same
    expression with every term in fp32, as the device's table (terms of several thousand at total_count = 255)."""
    from cirkit_amd import _capi as capi

    g = torch.Generator().manual_seed(total_count + is_logits)
    F, K = 3, 37
    if is_logits:
        p = torch.rand(F, K, generator=g) * 60 - 30
        p[0, :4] = torch.tensor([-30.0, 30.0, 0.0, 1e-3])
    else:
        p = torch.rand(F, K, generator=g)
        p[0, :3] = torch.tensor([1e-7, 0.5, 1 - 1e-7])
    o = _Guarded(F * (total_count + 2) * K, hip_device)
    capi.call("ck_param_binomial_table", p.to(hip_device).data_ptr(), is_logits, o.out.data_ptr(), F, K, total_count, _stream(hip_device))
    torch.cuda.synchronize()
    got = o.read().view(F, total_count + 2, K)
    assert bool((got[:, total_count + 1] == 0).all()), "the integral row is not exactly 0"
    assert bool(torch.isfinite(got).all())
    ref, yard = binomial_table(p.double(), bool(is_logits), total_count), binomial_table(p, bool(is_logits), total_count)
    _check_log("binomial", f"n={total_count} {'logits' if is_logits else 'probs'}", got, ref, yard, cut=-1e30)


# ---------------------------------------------------------------------------------------------- the host's guards
def _cat_plan(K, C, features=2):
    from cirkit_amd.templates import tabular_data

    return tabular_data(num_features=features, input_layers={"name": "categorical", "args": {"num_categories": C}},
                        num_input_units=K, num_sum_units=K if features > 2 else 4)


def _forward_vs_oracle(dev, plan, **kw):
    from cirkit_amd.circuit import HipCircuit
    from cirkit_amd.initializers import init_plan_tensors
    from oracle.torch_oracle import as_torch, evaluate_plan

    tensors = init_plan_tensors(plan)
    C = max(int(l.config["num_categories"]) for l in plan.layers if l.type == "categorical")
    g = torch.Generator().manual_seed(C)
    x = torch.randint(0, C, (8, plan.num_variables), generator=g)
    x[0, 0], x[1, 0] = 0, C - 1
    hc = HipCircuit(plan, tensors, device=dev, batch_params=True, **kw)
    y = hc(x.to(dev)).cpu().double()
    want = evaluate_plan(plan, {k: v.double() for k, v in as_torch(tensors).items()}, x)
    assert y.shape == want.shape and bool(torch.isfinite(y).all())
    assert float((y - want).abs().max()) <= 1e-5 * float(want.abs().max()), float((y - want).abs().max())
    return hc


@pytest.mark.parametrize("K,C,batched", [(128, 300, True), (128, 314, True), (128, 315, False), (128, 316, False), (128, 318, False),
                                         (64, 630, True), (64, 631, False), (64, 636, False)])
def test_categorical_guard_is_the_launchers_bound(hip_device, K, C, batched):
    """A Categorical layer registers its table job exactly when the launcher takes it (`ck_param_table_job_fits`: K (C + 4)
    + 2 K words and C (K + 1) in 160 KB; the host used to count K (C + 1) + 2 K and registered (128, 315 .. 317) and (64, 631 ..
    637), which the launch then refused: the forward raised).  Above the bound the layer takes the per-node kernels; the
    log-likelihood matches the oracle either way."""
    from cirkit_amd import _capi as capi
    from cirkit_amd.layers import HipCategoricalLayer

    assert capi.table_job_fits(1, C, K) == batched
    hc = _forward_vs_oracle(hip_device, _cat_plan(K, C))
    cats = [l for l in hc.layers if isinstance(l, HipCategoricalLayer)]
    assert cats and all(l._batched == batched for l in cats)
    kinds = [m["kind"] for m in hc._batch._meta]
    assert (1 in kinds) == batched


@pytest.mark.parametrize("C,fused", [(1242, True), (1243, False)])
def test_dense_on_table_guard_is_the_launchers_bound(hip_device, C, fused):
    """The kind 4 / 5 jobs of `HipCircuit` (a dense layer applied to its Categorical layer's table) are registered under the
    same bound: 32 (C + 4) + 64 + 1024 words fit up to C = 1242; at 1243 the circuit evaluates the layers on their own."""
    from cirkit_amd import _capi as capi

    assert capi.table_job_fits(5, C, 32) == fused and capi.table_job_fits(4, C, 32) == fused
    hc = _forward_vs_oracle(hip_device, _cat_plan(32, C, features=8))
    kinds = [m["kind"] for m in hc._batch._meta]
    assert any(k in (4, 5) for k in kinds) == fused, kinds
