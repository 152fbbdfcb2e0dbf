"""The top-down message pass kernel by kernel: the 16 entry points `ck_flow_*`, `ck_loo_*` and `ck_stats_*` (ck_down.h, ck_flow.hip,
ck_loo.hip, ck_stats.hip) through the C ABI on raw guarded buffers against the fp64 run of tests/topdown_restatement.py (pinned to
torch autograd by tests/test_topdown_restatement.py), on both sides of every boundary of the launchers.

The shapes are read off the launchers at this commit (nothing asserts which kernel ran):
* `launch_down_sum` (ck_down.h:194-221), behind `ck_flow_down_sum` and `ck_loo_down_sum`: `down_sum_mfma<32|64>` for a sum or CP-T
  layer that is not mixing with Ko = 32 / 64 and Ki % 32 == 0 (204-211), four (fold, 32 rows) tiles per workgroup (206: F row_tiles
  not a multiple of 4 leaves idle waves); else `down_sum_generic` with TR = 16 rows per workgroup halved while
  TR (Ko + 1 [+ Ki^2 for Tucker]) words exceed 48 KB (212-214: 768 words keep 16; Tucker Ki = 27 | 28, 38 | 39, 54 | 55, 77 | 78
  straddle 16/8, 8/4, 4/2, 2/1; a sum of Ko = 767 | 768, Ki = 1 straddles 16/8) and refused when one row does not fit (215:
  Tucker Ki = 111).  `test_down_sum_mfma`, `test_down_sum_generic`, `test_down_sum_tucker_by_lds_budget`,
  `test_down_sum_wide_sum`, `test_down_sum_refuses_past_the_lds_budget`.
* `launch_segment` (ck_down.h:223-235) and the product launches (ck_flow.hip:249-265, ck_loo.hip:294-307): one thread per
  (child, row, unit), ceil(n_child B Ki / 256) workgroups.  `test_segment`, `test_product`.
* `ck_flow_leaf_categorical` (ck_flow.hip:286-308): `flow_leaf_cat_mfma<32|64>` for K_uniform = 32 / 64 (296-303: a workgroup per
  (variable, 32 rows), its four waves the 32-state tiles, so Cout = 129 gives wave 0 a second tile and 256 every wave one), else
  the generic kernel (304-307).  `test_flow_leaf_categorical`.
* `ck_loo_leaf_categorical` (ck_loo.hip:309-322): a wave per (row, variable), four per workgroup (318), 4 max_units floats of
  LDS per wave, refused above 48 KB (316-317: max_units = 3072 | 3073).  `test_loo_leaf_categorical`.
* `ck_stats_edge_sum` (ck_stats.hip:358-411): `stats_edge_mfma` on the shapes of the down-sum (370), else `stats_edge_generic`
  with PC = ceil(Ko M / 1024) pair chunks (371) and TR = 16 halved by (Ko + M + 1) words a row (385-388: Tucker Ki = 27 | 28);
  S = min(ceil(1024 / tiles), ceil(B / 64)) row slices of an even number of rows when tiles < 1024, else 1 (347-354, 373-375:
  B = 64 | 65 gives 1 | 2, B = 129 gives 3 with an odd last pair, 171 folds of 6 tiles give 1), scratch of exactly tiles S 1024
  floats (376), a second launch adds the slices (405-407).  `test_stats_edge_*`.
* `ck_stats_leaf_categorical` (ck_stats.hip:413-430): KU = min(K, 256) units per workgroup halved (rounding up) while KU (C + 1)
  words exceed 48 KB (420-421: K = 64, C = 256 gives 32; K = 300, C = 40 gives 256 then a block of 44; K = 75, C = 256 gives
  38, which does not divide 256: 6 state groups, 28 idle threads), 256 / KU state groups of ceil(C / groups) states (423-424).
  `test_stats_leaf_categorical`.
* `ck_stats_unit_sum` (ck_stats.hip:313-345, 445-454): a workgroup per fold, 256 / Ko row groups for Ko <= 256, else a thread per
  unit in steps of 256.  `test_stats_unit_sum`.
* the remaining entry points launch one thread per output element, ceil(n / 256) workgroups: `test_flow_leaf_gaussian`,
  `test_flow_check_evidence`, `test_loo_leaf_gaussian_and_log_probs`, `test_stats_leaf_gaussian`.

Memory.  The message buffer is a `_Guarded`: every word of every slot of the launch must be written, every word outside keep the
NaN pattern.  The flow / derivative arena is a `_GuardedArena` laid out as the value arena, with the parent blocks and a prior
in every child block: the targeted child blocks must be fully written and every other word come back bit for bit (the parent
blocks the product kernels read from the same arena included); the down-sum launches must leave both arenas untouched.  `edge`,
`leaf` and `unit` carry a random prior; `scratch` is exactly the tiles S 1024 floats the launcher asks for, between guards.

Tolerance (the convention of tests/test_gpu_layer_backward.py).  The yardstick of a case is the error of the SAME restated
function run in fp32 on the CPU against its fp64 run on the case's own inputs; the GPU must be within 4 x that, with a floor of
1e-6.  Nothing in a bar comes from what the GPU returns, no finite entry is left out, NaN and -inf reference entries are matched
exactly.  In the 'far-tail' family the yardstick is the exact-shift fp32 run (topdown_restatement.EXACT32), not the plain one.
* Flow-space outputs (messages, arena, edge, leaf, unit, the categorical posteriors) are sums of non-negative terms: every entry
  is compared relative to its own fp64 value.  An entry may additionally be off by the fp64 sum of those of its terms whose
  shifted factor f_k exp(-v_k - m) is below 2^-120 in fp64 (what an fp32 factor cannot hold; from the inputs alone).  ONE
  allowance beyond the issue's: a non-zero entry may also be off by 2^-120 absolute.  The output is an fp32 number, which holds
  no relative precision below the smallest normal 2^-126, and T_i exp(m + e_i) with T_i up to Ko = 64 is computed through an
  exponential that is itself subnormal below 2^-126: 64 x 2^-126 = 2^-120 ('spread' and 'over80e' have such entries; a value
  of 2^-120 is 1e-36 of the row's flow).  Both allowances are taken off the yardstick's error too.  An entry that is exactly 0
  in fp64 (T_i = 0, e_i = -inf, a dead row) must be exactly 0.
* Log-space outputs (the derivative pass) are compared as logs, the absolute difference, where the fp64 entry is within 60 nats of
  its row's maximum, and in linear space relative to that maximum below; there -inf for a finite reference is legitimate.
* Normalised conditionals are compared relative to max|row| of the fp64 result; the Gaussian moments each on a scale of its
  own: sum_k p_k |mean_k| for the mean (a sum of terms of both signs: an fp32 evaluation is good to that, not to |S1|, which
  cancellation can leave arbitrarily small) and S2 + S1^2 for the variance S2 - S1^2.
`ck_flow_segment_add` and the flow pass's Hadamard add in list order, one fp32 rounding each: bit equality with the fp32 run.

Measured first (LAB_NOTES.md, "Top-down pass"): with torch's blocked matrix product in the fp32 run, `ck_flow_down_sum` stood at
4.46 x on the sum of Ko = 768 units (err 1.34e-6, yardstick 3.0e-7) and everything else within 3.2 x.  `down_sum_generic` adds the
Ko products of an entry in unit order, one fmaf each (ck_down.h:99); the fp32 run of the restatement now does the same, a plain
loop over the units, and gives 1.34e-6 there itself.  No allowance was added for it, and none anywhere else.

Value families.  The down-sum kernels and `ck_stats_edge_sum` run over 'normal', 'far-tail', 'spread', 'dropped', 'dead-row' and
'wzero' of `topdown_restatement.SumCase`, each down-sum followed by its segment launch on the messages the GPU wrote; the flow
down-sum over 'over80' / 'over80e' (-v_k - m and m + e_i on both sides of 80), `ck_stats_edge_sum` over 'kslow' (e_i + m on both
sides of 40).  These families are properties of a layer's forward.  `ck_loo_down_product`, which reads both arenas, runs over
'far-tail' (D + 700, values - 700 / H) and 'spread' arenas of its own next to 'normal' and 'neginf'; the kernels that read only
flows (`ck_flow_down_product`, the flow leaves, the statistics of the leaves and of the units) over uniform and 'spread' flows
(over e^-60) with zeros and dead rows; the derivative leaves over derivatives around 700 with -inf entries.
`test_two_sum_exponent_is_kept` is a bar on top of the convention: see its docstring.

Every case prints `TOPDOWN <entry point> <case> err yard ratio` (ratio = err / max(yard, floor / 4): a case passes iff ratio <= 4);
the worst per entry point are in LAB_NOTES.md, "Top-down pass"."""
import numpy as np
import pytest
import torch

import topdown_restatement as R
from guarded_buffers import NAN_BITS, NEG_INF, _Guarded, _GuardedArena, _stream

pytestmark = pytest.mark.gpu

FLOOR = 1e-6
TINY = 2.0 ** -120
F64, F32 = torch.float64, torch.float32
WORST: dict[str, tuple] = {}
CASES: dict[str, int] = {}
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for kernel in sorted(WORST):
        r, case, err, yard = WORST[kernel]
        print(f"\nTOPDOWN-WORST {kernel}: ratio {r:.3f} (err {err:.3e}, yardstick {yard:.3e}) at {case}; {CASES[kernel]} cases")
    print(f"\nTOPDOWN-CASES {sum(CASES.values())}")


def _dev(a, dev):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.contiguous().to(dev) if isinstance(a, torch.Tensor) else a


def _status(dev, name, *args):
    """The entry point on the current stream, then a synchronize; returns nothing, raises on a non-zero status.  Host tensors and
    numpy arrays among `args` are copied to the device and kept alive until the launch has finished."""
    from cirkit_amd import _capi as capi

    held = [_dev(a, dev) for a in args]
    capi.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in held], _stream(dev))
    torch.cuda.synchronize()


def _report(kernel, case, err, yard):
    err, yard = float(err), float(yard)
    ratio = err / max(yard, FLOOR / 4)
    print(f"TOPDOWN {kernel} {case} err {err:.3e} yard {yard:.3e} ratio {ratio:.3f}")
    CASES[kernel] = CASES.get(kernel, 0) + 1
    if kernel not in WORST or ratio > WORST[kernel][0]:
        WORST[kernel] = (ratio, case, err, yard)
    assert err <= max(4 * yard, FLOOR), f"{kernel} {case}: error {err:.3e} above 4 x the fp32 yardstick {yard:.3e} (floor {FLOOR})"


def _same_special(kernel, case, got, ref):
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{kernel} {case}: NaN where the reference has none (or the reverse)"
    inf = torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf]), f"{kernel} {case}: an infinite reference entry is not matched"


def _check_flow(kernel, case, got, ref, yard, allow=None):
    """Sums of non-negative terms, entry by entry relative to the entry's own fp64 value; `allow`: the fp64 sum of the terms an
    fp32 factor cannot hold.  An entry whose fp64 value is exactly 0 must be exactly 0."""
    got, yard = got.double().reshape(ref.shape), yard.double().reshape(ref.shape)
    _same_special(kernel, case, got, ref)
    extra = TINY if allow is None else allow.reshape(ref.shape) + TINY
    fin = torch.isfinite(ref)
    assert bool(torch.isfinite(got[fin]).all()), f"{kernel} {case}: non-finite where the reference is finite"
    assert bool(torch.isfinite(yard[fin]).all()), f"{kernel} {case}: the fp32 yardstick run is not finite where the fp64 run is"
    zero = torch.zeros((), dtype=F64)
    scale = torch.where(ref.abs() > 0, ref.abs(), torch.ones_like(ref))

    def err(x):
        d = torch.where(fin, ((x - ref).abs() - extra).clamp(min=0), zero)
        return (d / scale).max() if d.numel() else zero

    assert bool((got[fin & (ref == 0)] == 0).all()), f"{kernel} {case}: an entry that is exactly 0 in fp64 is not exactly 0"
    _report(kernel, case, err(got), err(yard))


def _check_log(kernel, case, got, ref, yard):
    """Logs: as logs within 60 nats of the row's maximum, in linear space relative to that maximum below."""
    got, yard = got.double().reshape(ref.shape), yard.double().reshape(ref.shape)
    _same_special(kernel, case, got, ref)
    fin = torch.isfinite(ref)
    ninf = torch.full_like(ref, NEG_INF)
    mx = torch.where(fin, ref, ninf).amax(-1, keepdim=True)
    mxs = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    near = fin & (ref >= mxs - 60)
    assert bool(torch.isfinite(got[near]).all()), f"{kernel} {case}: not finite within 60 nats of the row's maximum"
    assert bool(torch.isfinite(yard[near]).all()), f"{kernel} {case}: the fp32 yardstick run is not finite where the fp64 run is"
    assert not bool(torch.isnan(got[fin]).any()) and not bool((got[fin] == float("inf")).any())
    zero = torch.zeros((), dtype=F64)

    def err(x):
        xs = torch.where(near, x, ref)
        log_e = torch.where(near, (xs - ref).abs(), zero)
        lin_e = torch.where(fin & ~near, (torch.exp(torch.where(fin, x, ninf) - mxs) - torch.exp(torch.where(fin, ref, ninf) - mxs)).abs(), zero)
        return torch.maximum(log_e, lin_e).max() if x.numel() else zero

    _report(kernel, case, err(got), err(yard))


def _check_rows(kernel, case, got, ref, yard):
    """Relative to max|row| of the fp64 result (moments, normalised conditionals)."""
    got, yard = got.double().reshape(ref.shape), yard.double().reshape(ref.shape)
    _same_special(kernel, case, got, ref)
    fin = torch.isfinite(ref)
    assert bool(torch.isfinite(got[fin]).all()), f"{kernel} {case}: non-finite where the reference is finite"
    a = torch.where(fin, ref.abs(), torch.zeros_like(ref)).amax(-1, keepdim=True)
    s = torch.where(a > 0, a, torch.ones_like(a))
    zero = torch.zeros((), dtype=F64)
    _report(kernel, case, torch.where(fin, (got - ref).abs() / s, zero).max(), torch.where(fin, (yard - ref).abs() / s, zero).max())


def _bits(x):
    return x.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------- arenas
def _split(flat, sizes, off):
    return [flat[int(o):int(o) + int(n)] for o, n in zip(off, sizes)]


def _arena(dev, sizes, off, flat):
    a = _GuardedArena(sizes, dev)
    assert a.off == [int(o) for o in off], "the case's offsets are not the guarded arena's"
    host = a.fill(_split(flat, sizes, off))
    return a, host


def _yard_mode(fam):
    return R.EXACT32 if fam == "far-tail" else F32


# ----------------------------------------------------------------------------------- ck_flow_down_sum / ck_loo_down_sum
TYPE_NAME = {R.SUM: "sum", R.CPT: "cpt", R.TUCKER: "tucker"}


def _down_args(c):
    return (c.type, c.diag, c.child, c.w, c.F, c.H, c.Ki, c.Ko, c.M)


def _run_down(dev, c, rows=None):
    """One launch of the case's down-sum (on the row range `rows` of every block: a chunk of the batch); returns the message
    buffer (slots, rows, Ki) after the memory checks."""
    r0, r1 = rows if rows is not None else (0, c.B)
    nb = r1 - r0
    sizes = [n // c.B * nb for n in c.sizes]
    off, _ = R.arena_offsets(sizes)

    def rows_of(flat):
        out = torch.full((R.arena_offsets(sizes)[1],), NAN)
        for g, n in enumerate(c.sizes):
            K = n // c.B
            R.block(out, off, g, nb, K).copy_(R.block(flat, c.val_off, g, c.B, K)[r0:r1])
        return out

    va, _ = _arena(dev, sizes, off, rows_of(c.vals))
    aa, _ = _arena(dev, sizes, off, rows_of(c.arena))
    msg = _Guarded(R.n_slots(c.type, c.F, c.H, c.flow_pass) * nb * c.Ki, dev)
    name = "ck_flow_down_sum" if c.flow_pass else "ck_loo_down_sum"
    _status(dev, name, *_down_args(c), va.ptr(), aa.ptr(), np.array(off, dtype=np.int64), c.fold_off, nb, msg.out.data_ptr())
    got = msg.read().view(-1, nb, c.Ki)  # (every word of every slot written, the guards intact)
    va.read([])
    aa.read([])  # (both arenas bit for bit)
    return got


def _down_case(dev, kernel, flow_pass, type, diag, F, H, Ki, Ko, B, fam="normal", fold_off=0, seed=0, twice=False):
    g = torch.Generator().manual_seed(seed)
    c = R.SumCase(type, diag, F, H, Ki, Ko, B, fam, g, fold_off=fold_off, flow_pass=flow_pass)
    case = f"{TYPE_NAME[type]}{'(mixing)' if diag else ''} F={F} H={H} Ki={Ki} Ko={Ko} B={B} fold_off={c.fold_off} {fam}"
    got = _run_down(dev, c)
    fn = R.flow_down_sum if flow_pass else R.loo_down_sum
    args = (*_down_args(c), c.vals, c.arena, c.val_off, c.fold_off, B)
    ref, yard = fn(*args, F64), fn(*args, _yard_mode(fam))
    name = ("ck_flow_down_sum:" if flow_pass else "ck_loo_down_sum:") + kernel
    if flow_pass:
        _check_flow(name, case, got, ref, yard, fn(*args, F64, small=True))
    else:
        _check_log(name, case, got, ref, yard)
    if twice:
        assert torch.equal(_bits(_run_down(dev, c)), _bits(got)), f"{name} {case}: a second call is not bit-identical"
        if B > 32:
            parts = torch.cat([_run_down(dev, c, (0, 32)), _run_down(dev, c, (32, B))], dim=1)
            assert torch.equal(_bits(parts), _bits(got)), f"{name} {case}: the rows in two calls split at row 32 are not bit-identical"
    return c, got


def _segment_after(dev, c, msg, fam):
    """The segment launch that follows the case's down-sum, on the messages the GPU wrote: children 0 and 2 stored, child 1
    combined with its prior."""
    name = "ck_flow_segment_add" if c.flow_pass else "ck_loo_segment_lse"
    tables = c.csr([1, 0, 1][:c.nc])
    aa, _ = _arena(dev, c.sizes, c.val_off, c.arena)
    _status(dev, name, msg, *tables, aa.ptr(), c.val_off, c.nc, c.Ki, c.B)
    out = aa.read(c.cfolds)  # (the parents' blocks and the guards bit for bit)
    fn = R.flow_segment_add if c.flow_pass else R.loo_segment_lse
    ref, yard = (fn(msg, *tables, c.arena, c.val_off, c.nc, c.Ki, c.B, dt) for dt in (F64, F32))
    pick = lambda flat: torch.stack([R.block(flat, c.val_off, g, c.B, c.Ki) for g in c.cfolds])
    case = f"after {TYPE_NAME[c.type]} Ki={c.Ki} Ko={c.Ko} B={c.B} {fam}"
    if c.flow_pass:
        assert torch.equal(_bits(pick(out)), _bits(pick(yard))), f"{name} {case}: not the additions in list order, one fp32 rounding each"
        _check_flow(name, case, pick(out), pick(ref), pick(yard))
    else:
        _check_log(name, case, pick(out), pick(ref), pick(yard))


PASSES = [True, False]


@pytest.mark.parametrize("flow_pass", PASSES)
@pytest.mark.parametrize("Ki,Ko", [(32, 32), (64, 64), (96, 32), (32, 64)])
def test_down_sum_mfma(hip_device, flow_pass, Ki, Ko):
    """The matrix-core path: sum with H = 1, 2, 3 and CP-T with H = 2, 3; B on both sides of the 32-row tile; F = 3 (and 5 at
    B = 65: 15 tiles) leaves the last workgroup with idle waves; fold_off 0 and 3."""
    i = 0
    for type, H in ((R.SUM, 1), (R.SUM, 2), (R.SUM, 3), (R.CPT, 2), (R.CPT, 3)):
        for B in (1, 31, 32, 33, 65):
            F = 5 if B == 65 else 3
            _down_case(hip_device, f"mfma{Ko}", flow_pass, type, 0, F, H, Ki, Ko, B, fold_off=3 if i % 2 else 0, seed=Ki + Ko + H + B,
                       twice=B in (33, 65))
            i += 1


@pytest.mark.parametrize("flow_pass", PASSES)
def test_down_sum_generic(hip_device, flow_pass):
    """The plain path: Ko = 32 with Ki = 5 (no multiple of 32), mixing at K = 32 (it must not take the matrix cores: its weight
    is read on the block diagonals only, the rest holds random numbers) and K = 6, (1, 1), (7, 5), (33, 32); B on both sides of
    the 16-row tile."""
    i = 0
    for type, diag, H, Ki, Ko in ((R.SUM, 0, 2, 5, 32), (R.SUM, 1, 2, 32, 32), (R.SUM, 1, 3, 6, 6), (R.SUM, 0, 1, 1, 1), (R.SUM, 0, 2, 7, 5),
                                  (R.CPT, 0, 2, 7, 5), (R.SUM, 0, 2, 33, 32), (R.CPT, 0, 3, 33, 32), (R.TUCKER, 0, 2, 4, 4)):
        for B in (1, 15, 16, 17):
            _down_case(hip_device, "generic", flow_pass, type, diag, 3, H, Ki, Ko, B, fold_off=3 if i % 2 else 0, seed=Ki + Ko + H + B)
            i += 1
    _down_case(hip_device, "generic", flow_pass, R.SUM, 1, 3, 2, 32, 32, 65, seed=1, twice=True)
    _down_case(hip_device, "generic", flow_pass, R.TUCKER, 0, 2, 2, 5, 5, 65, seed=2, twice=True)


@pytest.mark.parametrize("flow_pass", PASSES)
@pytest.mark.parametrize("K", [4, 27, 28, 38, 39, 54, 55, 77, 78])
def test_down_sum_tucker_by_lds_budget(hip_device, flow_pass, K):
    """TR by Ko + 1 + Ki^2 words a row (ck_down.h:212-214): 16 up to K = 27, 8 up to 38, 4 up to 54, 2 up to 77, 1 at 78.
    B = 17 is a full tile of every TR and a ragged one."""
    _down_case(hip_device, "generic", flow_pass, R.TUCKER, 0, 2, 2, K, K, 17, seed=K)


@pytest.mark.parametrize("flow_pass", PASSES)
@pytest.mark.parametrize("Ko", [767, 768])
def test_down_sum_wide_sum(hip_device, flow_pass, Ko):
    """Ko + 1 = 768 words keep TR = 16, 769 halve it."""
    _down_case(hip_device, "generic", flow_pass, R.SUM, 0, 2, 1, 1, Ko, 17, seed=Ko)


@pytest.mark.parametrize("name", ["ck_flow_down_sum", "ck_loo_down_sum"])
def test_down_sum_refuses_past_the_lds_budget(hip_device, name):
    """Tucker Ki = 111: one row needs 111 + 1 + 12321 words, above 48 KB: -1 with the entry point's name, before any launch."""
    K, B = 111, 2
    off, words = R.arena_offsets([B * K] * 3)
    arena = torch.zeros(words)
    msg = _Guarded(2 * B * K, hip_device)
    with pytest.raises(ValueError, match=name + ": 111 units and 12321 entries exceed the LDS budget"):
        _status(hip_device, name, R.TUCKER, 0, np.array([1, 2], dtype=np.int32), torch.zeros(K * K * K), 1, 2, K, K, K * K, arena, arena,
                np.array(off, dtype=np.int64), 0, B, msg.out.data_ptr())
    assert bool((msg.raw() == NAN_BITS).all()), "a refused launch wrote something"


@pytest.mark.parametrize("fam,flow_pass", [(fam, True) for fam in R.FAMILIES + ["over80", "over80e"]] + [(fam, False) for fam in R.FAMILIES])
def test_down_sum_value_families(hip_device, flow_pass, fam):
    """Every value family through both kernels of both passes: B = 33 is a full tile and a ragged one of the matrix-core path,
    two tiles of the plain path and a ragged third.  'over80' / 'over80e' are the flow pass's: -v_k - m and m + e_i on both sides
    of 80 (`scaled_exp`'s fp64 branch)."""
    for kernel, type, diag, H, Ki, Ko in (("mfma32", R.SUM, 0, 2, 32, 32), ("mfma64", R.CPT, 0, 2, 64, 64), ("mfma32", R.CPT, 0, 3, 96, 32),
                                          ("generic", R.SUM, 0, 2, 7, 5), ("generic", R.CPT, 0, 2, 7, 5), ("generic", R.TUCKER, 0, 2, 6, 5),
                                          ("generic", R.SUM, 1, 2, 6, 6)):
        if diag and fam in ("wzero", "over80", "over80e"):
            continue  # (a mixing unit meets one entry per input: no entry to take from it, no heavier and lighter units of an entry)
        c, msg = _down_case(hip_device, kernel, flow_pass, type, diag, 2, H, Ki, Ko, 33, fam=fam, seed=len(fam) + Ki)
        _segment_after(hip_device, c, msg, fam)


@pytest.mark.parametrize("entry", ["ck_flow_down_sum", "ck_stats_edge_sum"])
def test_two_sum_exponent_is_kept(hip_device, entry):
    """On top of the bars above: ck_down.h promises x exp(a + b) "to ~2e-7 relative, whatever the size of a and b" (`scaled_exp`,
    `scaled_exp_core`: the exponent as an exact two-sum hi + lo, x exp(hi) (1 + lo)).  The plain and the exact-shift fp32 runs
    round the exponent once, which costs |a + b| 2^-25 relative -- 2e-6 on an entry e^-60 below its row's largest -- and so do
    not pin the promise; the TWOSUM32 run of the restatement keeps the remainder as the kernels say they do.  On the 'spread'
    family (exponents down to -90) the kernels must be within 4 x that run too, floor 1e-6."""
    for type, H, Ki, Ko in ((R.SUM, 2, 32, 32), (R.CPT, 2, 64, 64), (R.SUM, 2, 7, 5), (R.CPT, 2, 7, 5), (R.TUCKER, 2, 6, 5)):
        g = torch.Generator().manual_seed(Ki + Ko)
        c = R.SumCase(type, 0, 2, H, Ki, Ko, 33, "spread", g)
        case = f"{TYPE_NAME[type]} H={H} Ki={Ki} Ko={Ko} B=33 spread"
        if entry == "ck_flow_down_sum":
            args = (*_down_args(c), c.vals, c.arena, c.val_off, c.fold_off, 33)
            got = _run_down(hip_device, c)
            _check_flow(entry + ":two-sum", case, got, R.flow_down_sum(*args, F64), R.flow_down_sum(*args, R.TWOSUM32), R.flow_down_sum(*args, F64, small=True))
        else:
            live, prior = np.ones(33, dtype=np.int32), torch.zeros(2, Ko, c.M)
            args = (*_down_args(c), c.vals, c.arena, c.val_off, c.fold_off, live, 33, prior)
            got, _, _ = _edge_run(hip_device, c, live, prior)
            _check_flow(entry + ":two-sum", case, got, R.stats_edge_sum(*args, F64), R.stats_edge_sum(*args, R.TWOSUM32), R.stats_edge_sum(*args, F64, small=True))


# ----------------------------------------------------------------------------- ck_flow_segment_add / ck_loo_segment_lse
def _segment_tables(n_child, n_slots_):
    """Children with 1 .. 4 items, in turn; cfirst alternates; children j and j + 1 share a slot (one consumer, two children)."""
    cstart, items = [0], []
    for j in range(n_child):
        for t in range(j % 4 + 1):
            items.append((2 * j + 3 * t) % n_slots_)
        if j + 1 < n_child:
            items[-1] = (2 * (j + 1)) % n_slots_  # (the first item of the next child)
        cstart.append(len(items))
    return np.array(cstart, dtype=np.int32), np.array(items, dtype=np.int32), np.array([(j + 1) % 2 for j in range(n_child)], dtype=np.int32)


@pytest.mark.parametrize("flow_pass", PASSES)
@pytest.mark.parametrize("n_child,B,Ki", [(4, 1, 1), (4, 1, 6), (4, 1, 32), (8, 1, 32), (4, 33, 1), (4, 33, 6), (4, 33, 32), (3, 85, 1), (3, 43, 2)])
def test_segment(hip_device, flow_pass, n_child, B, Ki):
    """1 to 4 items per child, both values of cfirst in one launch, two children sharing a slot; n_child B Ki = 255, 256 and 258
    among others.  Child blocks in shuffled order in the arena, one block nobody targets.  Twice, and in two chunks of rows."""
    name = "ck_flow_segment_add" if flow_pass else "ck_loo_segment_lse"
    for fam in ("normal", "neginf"):
        g = torch.Generator().manual_seed(n_child + B + Ki)
        slots = 2 * n_child + 1
        cstart, items, cfirst = _segment_tables(n_child, slots)
        msg = torch.rand(slots, B, Ki, generator=g) if flow_pass else torch.randn(slots, B, Ki, generator=g) * 3 + 700
        if fam == "neginf":
            if flow_pass:
                msg[torch.rand(slots, B, Ki, generator=g) < 0.3] = 0.0
            else:
                msg[torch.rand(slots, B, Ki, generator=g) < 0.3] = NEG_INF
                msg[0] = NEG_INF
        order = torch.randperm(n_child + 1, generator=g).numpy()
        cfold = order[:n_child].astype(np.int32)
        sizes = [B * Ki] * (n_child + 1)
        off, words = R.arena_offsets(sizes)
        prior = torch.rand(words, generator=g) if flow_pass else torch.randn(words, generator=g) * 3 + 700
        if fam == "neginf" and not flow_pass:
            prior[torch.rand(words, generator=g) < 0.3] = NEG_INF
        fn = R.flow_segment_add if flow_pass else R.loo_segment_lse
        tables = (cstart, cfold, cfirst, items)
        ref, yard = fn(msg, *tables, prior, off, n_child, Ki, B, F64), fn(msg, *tables, prior, off, n_child, Ki, B, F32)

        def run(r0, r1):
            nb = r1 - r0
            sz = [nb * Ki] * (n_child + 1)
            o, w = R.arena_offsets(sz)
            flat = torch.full((w,), NAN)
            for b in range(n_child + 1):
                R.block(flat, o, b, nb, Ki).copy_(R.block(prior, off, b, B, Ki)[r0:r1])
            a, _ = _arena(hip_device, sz, o, flat)
            _status(hip_device, name, msg[:, r0:r1].contiguous(), *tables, a.ptr(), np.array(o, dtype=np.int64), n_child, Ki, nb)
            out = a.read([int(x) for x in cfold])
            return torch.stack([R.block(out, o, int(b), nb, Ki) for b in cfold])

        got = run(0, B)
        case = f"n_child={n_child} B={B} Ki={Ki} {fam}"
        pick = lambda flat: torch.stack([R.block(flat, off, int(b), B, Ki) for b in cfold])
        if flow_pass:
            assert torch.equal(_bits(got), _bits(pick(yard))), f"{name} {case}: not the additions in list order, one fp32 rounding each"
            _check_flow(name, case, got, pick(ref), pick(yard))
        else:
            _check_log(name, case, got, pick(ref), pick(yard))
        assert torch.equal(_bits(run(0, B)), _bits(got)), f"{name} {case}: a second call is not bit-identical"
        if B > 32:
            assert torch.equal(_bits(torch.cat([run(0, 32), run(32, B)], dim=1)), _bits(got)), f"{name} {case}: two chunks of rows are not bit-identical"


# --------------------------------------------------------------------------- ck_flow_down_product / ck_loo_down_product
CONSUMERS = {2: [[0, 1], [0, 2], [0, 1], [0, 3]], 3: [[0, 1, 2], [0, 2, 1], [0, 1, 1], [0, 3, 3]]}


@pytest.mark.parametrize("flow_pass", PASSES)
@pytest.mark.parametrize("type,H,Ki", [(R.HADAMARD, 2, 1), (R.HADAMARD, 2, 6), (R.HADAMARD, 3, 32), (R.KRONECKER, 2, 3), (R.KRONECKER, 2, 8),
                                       (R.KRONECKER, 3, 4)])
def test_product(hip_device, flow_pass, type, H, Ki):
    """Four consumers (global folds 2 .. 5, the layer's first fold is 2) over four child folds (0, 1, 6, 7) that receive 4, 2 or
    4, 1 or 2 and 1 or 2 items, at every input position, one of them from the same consumer twice; cfirst 1, 0, 1, 0.  B = 1 and
    33.  The consumers' blocks are read from the arena the children are written to: they must come back bit for bit.  'neginf':
    -inf child values (a -inf sibling of the derivative messages) and derivatives, zero flows.  'spread': flows over e^-60,
    derivatives and values over +-30.  'far-tail' (derivative pass): D about +700 and every value about -700 / H, the sizes
    under observed pixels, where the sibling additions (Hadamard in input order, Kronecker by digit) round at 2^-15 and the
    order they are taken in shows."""
    name = "ck_flow_down_product" if flow_pass else "ck_loo_down_product"
    Ko = Ki if type == R.HADAMARD else Ki ** H
    cid = [0, 1, 6, 7]
    for B in (1, 33):
        for fam in ("normal", "neginf", "spread") if flow_pass else ("normal", "neginf", "far-tail", "spread"):
            g = torch.Generator().manual_seed(H + Ki + B)
            sizes = [B * Ki] * 2 + [B * Ko] * 4 + [B * Ki] * 2
            off, words = R.arena_offsets(sizes)
            child = np.array([cid[j] for row in CONSUMERS[H] for j in row], dtype=np.int32)
            vals, arena = torch.full((words,), NAN), torch.full((words,), NAN)
            for c in cid:
                v = torch.randn(B, Ki, generator=g)
                p = torch.rand(B, Ki, generator=g) if flow_pass else torch.randn(B, Ki, generator=g) * 2
                if fam == "far-tail":
                    v, p = v - 700.0 / H, p + 700.0 / H
                if fam == "spread":
                    v = (torch.rand(B, Ki, generator=g) * 60 - 30) / H
                    p = torch.exp(-60 * torch.rand(B, Ki, generator=g)) if flow_pass else torch.rand(B, Ki, generator=g) * 60 - 30
                if fam == "neginf" and Ki > 1:
                    v[torch.rand(B, Ki, generator=g) < 0.15] = NEG_INF
                R.block(vals, off, c, B, Ki).copy_(v)
                R.block(arena, off, c, B, Ki).copy_(p)
            for p in range(2, 6):
                x = torch.rand(B, Ko, generator=g) if flow_pass else torch.randn(B, Ko, generator=g) * 2
                if fam == "far-tail":
                    x = x + 700.0
                if fam == "spread":
                    x = torch.exp(-60 * torch.rand(B, Ko, generator=g)) if flow_pass else torch.rand(B, Ko, generator=g) * 60 - 30
                if fam == "neginf":
                    x[torch.rand(B, Ko, generator=g) < 0.3] = 0.0 if flow_pass else NEG_INF
                    x[B // 2] = 0.0 if flow_pass else NEG_INF
                R.block(arena, off, p, B, Ko).copy_(x)
                R.block(vals, off, p, B, Ko).copy_(torch.randn(B, Ko, generator=g))
            cstart, pairs = [0], []
            for c in cid:
                pairs += [(2 + f, h) for f in range(4) for h in range(H) if child[f * H + h] == c]
                cstart.append(len(pairs))
            cstart, cfold, cfirst = np.array(cstart, dtype=np.int32), np.array(cid, dtype=np.int32), np.array([1, 0, 1, 0], dtype=np.int32)
            hada_flow = flow_pass and type == R.HADAMARD
            items = np.array([p[0] for p in pairs] if hada_flow else [x for p in pairs for x in p], dtype=np.int32)
            va, _ = _arena(hip_device, sizes, off, vals)
            aa, _ = _arena(hip_device, sizes, off, arena)
            o64 = np.array(off, dtype=np.int64)
            if flow_pass:
                _status(hip_device, name, type, cstart, cfold, cfirst, items, aa.ptr(), o64, 4, H, Ki, Ko, B)
                ref, yard = (R.flow_down_product(type, cstart, cfold, cfirst, items, arena, off, 4, H, Ki, Ko, B, dt) for dt in (F64, F32))
            else:
                _status(hip_device, name, type, cstart, cfold, cfirst, items, child, 2, va.ptr(), aa.ptr(), o64, 4, H, Ki, Ko, B)
                ref, yard = (R.loo_down_product(type, cstart, cfold, cfirst, items, child, 2, vals, arena, off, 4, H, Ki, Ko, B, dt) for dt in (F64, F32))
                va.read([])
            out = aa.read(cid)  # (the consumers' blocks and the guards bit for bit)
            pick = lambda flat: torch.stack([R.block(flat, off, c, B, Ki) for c in cid])
            case = f"{'hadamard' if type == R.HADAMARD else 'kronecker'} H={H} Ki={Ki} B={B} {fam}"
            if flow_pass:
                if type == R.HADAMARD:
                    assert torch.equal(_bits(pick(out)), _bits(pick(yard))), f"{name} {case}: not the additions in list order"
                _check_flow(name, case, pick(out), pick(ref), pick(yard))
            else:
                _check_log(name, case, pick(out), pick(ref), pick(yard))
            if not flow_pass and type == R.HADAMARD:
                # one item per child, stored: the message itself, D_g[k] plus the siblings' values ADDED IN INPUT ORDER, with no
                # logarithm in between -- bit for bit the fp32 run (at H = 3 and values of 700 any other order rounds differently)
                one = np.arange(5, dtype=np.int32)
                first = np.array([x for j in range(4) for x in pairs[int(cstart[j])]], dtype=np.int32)
                stored = np.ones(4, dtype=np.int32)
                aa, _ = _arena(hip_device, sizes, off, arena)
                _status(hip_device, name, type, one, cfold, stored, first, child, 2, va.ptr(), aa.ptr(), o64, 4, H, Ki, Ko, B)
                yard = R.loo_down_product(type, one, cfold, stored, first, child, 2, vals, arena, off, 4, H, Ki, Ko, B, F32)
                assert torch.equal(_bits(pick(aa.read(cid))), _bits(pick(yard))), f"{name} {case}: not D plus the siblings' values in input order"


# -------------------------------------------------------------------------------------------------------- flow leaves
def _leaf_tables(Ks, Cs, var_of, five):
    """entries (n, 4 | 5) of input folds 0 .. n - 1 (fold s over variable var_of[s], sorted), qstart, and the table sizes."""
    toff = np.cumsum([0] + [k * c for k, c in zip(Ks, Cs)])
    zoff = np.cumsum([0] + list(Ks))
    entries = np.array([[s, Ks[s], Cs[s], toff[s], zoff[s]][:5 if five else 4] for s in range(len(Ks))], dtype=np.int64)
    Q = max(var_of) + 1
    qstart = np.array([sum(1 for v in var_of if v < q) for q in range(Q + 1)], dtype=np.int32)
    return entries, qstart, int(toff[-1]), int(zoff[-1])


def _leaf_flow(B, K, g, fam):
    """(B, K) flows of an input fold: uniform with 20 % zeros; 'spread': over e^-60."""
    f = torch.exp(-60 * torch.rand(B, K, generator=g)) if fam == "spread" else torch.rand(B, K, generator=g)
    f[torch.rand(B, K, generator=g) < 0.2] = 0.0
    return f


BF = lambda Bs: [(B, fam) for B in Bs for fam in ("normal", "spread")]


def _check_scaled(kernel, case, got, ref, yard, scale):
    """Every entry on a scale of its own (fp64, from the inputs alone)."""
    got, yard = got.double().reshape(ref.shape), yard.double().reshape(ref.shape)
    _same_special(kernel, case, got, ref)
    fin = torch.isfinite(ref)
    assert bool(torch.isfinite(got[fin]).all()), f"{kernel} {case}: non-finite where the reference is finite"
    s = torch.where(fin & (scale > 0), scale, torch.ones_like(ref))
    zero = torch.zeros((), dtype=F64)
    _report(kernel, case, torch.where(fin, (got - ref).abs() / s, zero).max(), torch.where(fin, (yard - ref).abs() / s, zero).max())


def _moment_scale(ref, ref_abs_mean):
    """(.., 2) scales of (S1, S2 - S1^2): sum_k p_k |mean_k| for the mean, a sum of terms of both signs, and S2 + S1^2 for the
    variance, the two terms of its difference; `ref_abs_mean`: the fp64 run with |mean| in the place of mean (the same S2)."""
    s1, var = ref[..., 0], ref[..., 1]
    return torch.stack([ref_abs_mean[..., 0], var + 2 * s1 * s1], -1)


def _bad_rows(B, g):
    bad = (torch.rand(B, generator=g) < 0.2).to(torch.int32)
    if B > 2:
        bad[1] = 1
        bad[0] = 0
    return bad.numpy()


@pytest.mark.parametrize("K_uniform", [32, 64, 0])
@pytest.mark.parametrize("Cout", [2, 32, 33, 129, 256])
def test_flow_leaf_categorical(hip_device, K_uniform, Cout):
    """Two entries over variable 0 (the second with fewer states than Cout), one over variable 1; K_uniform = 0: units 5, 32, 7.
    B on both sides of the 32-row tile; rows with bad = 1 and rows with a -inf root among good ones; logev present and absent;
    flows uniform and spread over e^-60."""
    Ks = [K_uniform] * 3 if K_uniform else [5, 32, 7]
    Cs = [Cout, max(1, Cout // 2), Cout]
    entries, qstart, _, _ = _leaf_tables(Ks, Cs, [0, 0, 1], False)
    for B, fam in BF((1, 31, 32, 33)):
        g = torch.Generator().manual_seed(K_uniform + Cout + B)
        sizes = [B * k for k in Ks] + [B * 2]
        off, words = R.arena_offsets(sizes)
        flow, vals = torch.full((words,), NAN), torch.full((words,), NAN)
        for s in range(3):
            R.block(flow, off, s, B, Ks[s]).copy_(_leaf_flow(B, Ks[s], g, fam))
        root = torch.randn(B, 2, generator=g) - 700
        if B > 2:
            root[2, 0] = NEG_INF
        R.block(vals, off, 3, B, 2).copy_(root)
        ntab = torch.cat([torch.softmax(torch.randn(k, c, generator=g) * 3, -1).reshape(-1) for k, c in zip(Ks, Cs)])
        bad = _bad_rows(B, g)
        fa, _ = _arena(hip_device, sizes, off, flow)
        va, _ = _arena(hip_device, sizes, off, vals)
        for with_logev in (True, False):
            out, logev = _Guarded(B * 2 * Cout, hip_device), _Guarded(B, hip_device)
            _status(hip_device, "ck_flow_leaf_categorical", entries, qstart, 2, Cout, K_uniform, ntab, fa.ptr(), va.ptr(), np.array(off, dtype=np.int64),
                    3, 2, bad, B, out.out.data_ptr(), logev.out.data_ptr() if with_logev else None)
            (ref, lref), (yard, _) = (R.flow_leaf_categorical(entries, qstart, 2, Cout, ntab, flow, vals, off, 3, 2, bad, B, dt) for dt in (F64, F32))
            kernel = "ck_flow_leaf_categorical:" + (f"mfma{K_uniform}" if K_uniform else "generic")
            _check_flow(kernel, f"Cout={Cout} B={B} logev={int(with_logev)} {fam}", out.read().view(B, 2, Cout), ref, yard)
            if with_logev:
                got = logev.read()
                assert torch.equal(torch.isnan(got), torch.isnan(lref)) and torch.equal(got[~torch.isnan(got)].double(), lref[~torch.isnan(lref)])
            else:
                assert bool((logev.raw() == NAN_BITS).all())
        fa.read([])
        va.read([])


def _gauss_params(n, g):
    return torch.randn(n, generator=g) * 3, torch.exp(torch.rand(n, generator=g) * 4 - 3)


@pytest.mark.parametrize("B,fam", BF([1, 33, 130]))
def test_flow_leaf_gaussian(hip_device, B, fam):
    """The mean on the scale sum_k f_k |mean_k| and the variance on S2 + S1^2, each entry its own (`_moment_scale`)."""
    Ks = [5, 32, 7]
    entries, qstart, _, nz = _leaf_tables(Ks, [1, 1, 1], [0, 0, 1], True)
    entries = np.ascontiguousarray(entries[:, [0, 1, 2, 4]])  # (the offsets index mean / stddev)
    g = torch.Generator().manual_seed(B)
    sizes = [B * k for k in Ks] + [B]
    off, words = R.arena_offsets(sizes)
    flow, vals = torch.full((words,), NAN), torch.full((words,), NAN)
    for s in range(3):
        R.block(flow, off, s, B, Ks[s]).copy_(_leaf_flow(B, Ks[s], g, fam) / Ks[s])
    root = torch.randn(B, 1, generator=g)
    root[B // 2] = NEG_INF
    R.block(vals, off, 3, B, 1).copy_(root)
    mean, std = _gauss_params(nz, g)
    bad = _bad_rows(B, g)
    fa, _ = _arena(hip_device, sizes, off, flow)
    va, _ = _arena(hip_device, sizes, off, vals)
    out, logev = _Guarded(B * 2 * 2, hip_device), _Guarded(B, hip_device)
    _status(hip_device, "ck_flow_leaf_gaussian", entries, qstart, 2, mean, std, fa.ptr(), va.ptr(), np.array(off, dtype=np.int64), 3, 1, bad, B,
            out.out.data_ptr(), logev.out.data_ptr())
    (ref, lref), (yard, _) = (R.flow_leaf_gaussian(entries, qstart, 2, mean, std, flow, vals, off, 3, 1, bad, B, dt) for dt in (F64, F32))
    scale = _moment_scale(ref, R.flow_leaf_gaussian(entries, qstart, 2, mean.abs(), std, flow, vals, off, 3, 1, bad, B, F64)[0])
    _check_scaled("ck_flow_leaf_gaussian", f"B={B} {fam}", out.read().view(B, 2, 2), ref, yard, scale)
    got = logev.read()
    assert torch.equal(torch.isnan(got), torch.isnan(lref)) and torch.equal(got[~torch.isnan(got)].double(), lref[~torch.isnan(lref)])


@pytest.mark.parametrize("x_float", [0, 1])
@pytest.mark.parametrize("B,D", [(1, 3), (33, 3), (130, 5)])
def test_flow_check_evidence(hip_device, x_float, B, D):
    """B D on both sides of the 256 threads; sentinels, in-range and out-of-range categories, a variable no discrete layer reads
    (states 0).  clean lies between guards of its own dtype; bad is only ever set; the flag is or-ed."""
    g = torch.Generator().manual_seed(B + D)
    states = np.array([3, 0, 5, 2, 7][:D], dtype=np.int32)
    ev = torch.randint(-2, 9, (B, D), generator=g)
    ev[0] = torch.tensor([2, 8, 4, 1, 6][:D])  # (a clean row)
    x = ev.float() if x_float else ev
    if x_float:
        x[torch.rand(B, D, generator=g) < 0.1] = NAN
        x = torch.where((x >= 0) & (torch.rand(B, D, generator=g) < 0.5), x + 0.5, x)  # (2.5 is category 2; 2.5 >= states 3 is not)
    pad = 16
    clean = torch.full((B * D + 2 * pad,), 77, dtype=x.dtype).to(hip_device)
    bad, flag = torch.zeros(B + 2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32).to(hip_device)
    bad[1] = 1  # (row 0, a clean row, was marked before: it must stay marked)
    bad = bad.to(hip_device)
    _status(hip_device, "ck_flow_check_evidence", x, x_float, states, B, D, clean[pad:].data_ptr(), bad[1:].data_ptr(), flag[1:].data_ptr())
    wc, wb, wf = R.flow_check_evidence(x, x_float, states, B, D)
    c = clean.cpu()
    assert bool((c[:pad] == 77).all()) and bool((c[pad + B * D:] == 77).all())
    gotc = c[pad:pad + B * D].view(B, D)
    assert torch.equal(torch.isnan(gotc), torch.isnan(wc)) if x_float else True
    assert torch.equal(torch.nan_to_num(gotc.double(), nan=-5.0), torch.nan_to_num(wc.double(), nan=-5.0))
    assert int(wb[0]) == 0
    assert bad.cpu().tolist() == [0, 1] + wb.tolist()[1:] + [0] and flag.cpu().tolist() == [0, wf, 0]


# -------------------------------------------------------------------------------------------------- derivative leaves
def _der_arena(Ks, B, g, shift=0.0, extra=()):
    sizes = [B * k for k in Ks] + list(extra)
    off, words = R.arena_offsets(sizes)
    der, vals = torch.full((words,), NAN), torch.full((words,), NAN)
    for s, K in enumerate(Ks):
        d = torch.randn(B, K, generator=g) * 4 + shift
        d[torch.rand(B, K, generator=g) < 0.2] = NEG_INF
        R.block(der, off, s, B, K).copy_(d)
        R.block(vals, off, s, B, K).copy_(torch.randn(B, K, generator=g) * 3 - shift)
    return sizes, off, der, vals


@pytest.mark.parametrize("units", [1, 70, 3072])
def test_loo_leaf_categorical(hip_device, units):
    """max_units = 1 (one unit), 70 (32 + 38 over variable 0) and 3072 (three folds of 1024: the whole 48 KB); B Q = 3, 6 and 66:
    a ragged last workgroup and full ones.  The other variable has one fold with fewer states than Cout.  -inf derivatives, a
    log Z of -inf, a (row, variable) without mass, rows with bad = 1; derivatives around 700 (the size they have under observed
    pixels)."""
    Ks = {1: [1, 1], 70: [32, 38, 5], 3072: [1024, 1024, 1024, 3]}[units]
    var_of = {1: [0, 1], 70: [0, 0, 1], 3072: [0, 0, 0, 1]}[units]
    Cout = 2 if units == 3072 else 33
    Cs = [Cout] * (len(Ks) - 1) + [max(1, Cout // 2)]
    entries, qstart, _, nz = _leaf_tables(Ks, Cs, var_of, True)
    for B in ((3,) if units == 3072 else (3, 33)):
        g = torch.Generator().manual_seed(units + B)
        sizes, off, der, _ = _der_arena(Ks, B, g, shift=700.0)
        if units > 1:
            R.block(der, off, len(Ks) - 1, B, Ks[-1])[B // 2] = NEG_INF  # (no mass)
        ntab = torch.cat([torch.softmax(torch.randn(k, c, generator=g) * 3, -1).reshape(-1) for k, c in zip(Ks, Cs)])
        lz = torch.randn(nz, generator=g) * 2
        if units > 1:
            lz[1] = NEG_INF
        bad = _bad_rows(B, g)
        da, _ = _arena(hip_device, sizes, off, der)
        out = _Guarded(B * 2 * Cout, hip_device)
        _status(hip_device, "ck_loo_leaf_categorical", entries, qstart, 2, Cout, units, ntab, lz, da.ptr(), np.array(off, dtype=np.int64), bad, B,
                out.out.data_ptr())
        ref, yard = (R.loo_leaf_categorical(entries, qstart, 2, Cout, ntab, lz, der, off, bad, B, dt) for dt in (F64, F32))
        _check_rows("ck_loo_leaf_categorical", f"max_units={units} B={B}", out.read().view(B, 2, Cout), ref, yard)
        da.read([])


def test_loo_leaf_categorical_refuses_past_the_lds_budget(hip_device):
    out = _Guarded(4, hip_device)
    z = torch.zeros(64)
    with pytest.raises(ValueError, match="ck_loo_leaf_categorical: 3073 input units over one variable exceed the LDS budget"):
        _status(hip_device, "ck_loo_leaf_categorical", np.zeros((1, 5), dtype=np.int64), np.array([0, 1], dtype=np.int32), 1, 2, 3073, z, z, z,
                np.zeros(1, dtype=np.int64), np.zeros(2, dtype=np.int32), 2, out.out.data_ptr())
    assert bool((out.raw() == NAN_BITS).all()), "a refused launch wrote something"


@pytest.mark.parametrize("x_float", [0, 1])
@pytest.mark.parametrize("B", [1, 33, 130])
def test_loo_leaf_gaussian_and_log_probs(hip_device, B, x_float):
    """Three variables: 0 with two folds, 1 with one, 2 covered by no entry; vkind marks variable 1 Gaussian in the fp32 batch (NaN
    is its sentinel there).  Rows with bad = 1, a (row, variable) without a derivative, sentinels."""
    Ks = [5, 32, 7]
    entries, vstart, _, nz = _leaf_tables(Ks, [1, 1, 1], [0, 0, 1], True)
    vstart3 = np.array(list(vstart) + [int(vstart[-1])], dtype=np.int32)
    g = torch.Generator().manual_seed(B + x_float)
    sizes, off, der, vals = _der_arena(Ks, B, g, shift=700.0)
    R.block(der, off, 2, B, 7)[B // 2] = NEG_INF
    lz = torch.randn(nz, generator=g)
    bad = _bad_rows(B, g)
    mean, std = _gauss_params(nz, g)
    da, _ = _arena(hip_device, sizes, off, der)
    va, _ = _arena(hip_device, sizes, off, vals)
    o64 = np.array(off, dtype=np.int64)
    if x_float == 0:
        gent = np.ascontiguousarray(entries[:, [0, 1, 2, 4, 4]])
        out = _Guarded(B * 2 * 2, hip_device)
        _status(hip_device, "ck_loo_leaf_gaussian", gent, vstart, 2, mean, std, da.ptr(), o64, bad, B, out.out.data_ptr())
        ref, yard = (R.loo_leaf_gaussian(gent, vstart, 2, mean, std, der, off, bad, B, dt) for dt in (F64, F32))
        scale = _moment_scale(ref, R.loo_leaf_gaussian(gent, vstart, 2, mean.abs(), std, der, off, bad, B, F64))
        _check_scaled("ck_loo_leaf_gaussian", f"B={B}", out.read().view(B, 2, 2), ref, yard, scale)
    ev = torch.randint(-1, 4, (B, 3), generator=g)
    vkind = np.array([0, 2 if x_float else 0, 0], dtype=np.int32)
    x = ev
    if x_float:
        x = ev.float()
        x[:, 1] = torch.where(torch.rand(B, generator=g) < 0.3, torch.full((B,), NAN), torch.randn(B, generator=g))
    out = _Guarded(B * 3, hip_device)
    _status(hip_device, "ck_loo_log_probs", entries, vstart3, vkind, 3, lz, da.ptr(), va.ptr(), o64, x, x_float, bad, B, out.out.data_ptr())
    ref, yard = (R.loo_log_probs(entries, vstart3, vkind, 3, lz, der, vals, off, x, x_float, bad, B, dt) for dt in (F64, F32))
    got = out.read().view(B, 3)
    assert bool((got[:, 2][torch.as_tensor(bad) == 0] == 0).all()), "a variable no input layer covers is not exactly 0"
    # a difference of two log-sum-exps: an absolute error on a log, every column its own row
    _check_log("ck_loo_log_probs", f"B={B} x_float={x_float}", got.reshape(B * 3, 1), ref.reshape(B * 3, 1), yard.reshape(B * 3, 1))
    da.read([])
    va.read([])


# ---------------------------------------------------------------------------------------------------- ck_stats_edge_sum
def _slices(tiles, B):
    """S of ck_stats.hip:347-354, restated from the header of `ck_stats_edge_sum`."""
    return 1 if tiles >= 1024 else max(1, min(-(-1024 // tiles), -(-B // 64)))


def _live(B, kind, g):
    live = np.ones(B, dtype=np.int32)
    if kind == "none":
        live[:] = 0
    elif kind == "some":
        live[(torch.rand(B, generator=g) < 0.3).numpy()] = 0
        live[0] = 0  # (a dead row paired with a live one)
        if B > 1:
            live[1] = 1
        if B > 3:
            live[B - 1] = 0
    return live


def _edge_run(dev, c, live, prior):
    mfma = not c.diag and c.type != R.TUCKER and c.Ko in (32, 64) and c.Ki % 32 == 0
    tiles = c.F * (c.Ko // 32) * (c.M // 32) if mfma else c.F * -(-c.Ko * c.M // 1024)
    S = _slices(tiles, c.B)
    va, _ = _arena(dev, c.sizes, c.val_off, c.vals)
    fa, _ = _arena(dev, c.sizes, c.val_off, c.arena)
    edge = _Guarded(c.F * c.Ko * c.M, dev)
    edge.out.copy_(prior.reshape(-1))
    scratch = _Guarded(tiles * S * 1024, dev) if S > 1 else None
    _status(dev, "ck_stats_edge_sum", *_down_args(c), va.ptr(), fa.ptr(), c.val_off, c.fold_off, live, c.B, edge.out.data_ptr(),
            scratch.out.data_ptr() if scratch is not None else None, tiles * S * 1024 if scratch is not None else 0)
    if scratch is not None:
        scratch.read()  # (every partial tile written, nothing beyond)
    va.read([])
    fa.read([])
    return edge.read().view(c.F, c.Ko, c.M), S, mfma


def _edge_case(dev, type, diag, F, H, Ki, Ko, B, fam="normal", live_kind="some", fold_off=0, seed=0, twice=False):
    g = torch.Generator().manual_seed(seed)
    c = R.SumCase(type, diag, F, H, Ki, Ko, B, fam, g, fold_off=fold_off, flow_pass=True)
    live = _live(B, live_kind, g)
    prior = torch.rand(F, Ko, c.M, generator=g)
    got, S, mfma = _edge_run(dev, c, live, prior)
    args = (*_down_args(c), c.vals, c.arena, c.val_off, c.fold_off, live, B, prior)
    ref, yard, allow = R.stats_edge_sum(*args, F64), R.stats_edge_sum(*args, _yard_mode(fam)), R.stats_edge_sum(*args[:-1], torch.zeros_like(prior), F64, small=True)
    kernel = "ck_stats_edge_sum:" + (f"mfma{Ko}" if mfma else "generic")
    case = f"{TYPE_NAME[type]}{'(mixing)' if diag else ''} F={F} H={H} Ki={Ki} Ko={Ko} B={B} S={S} live={live_kind} {fam}"
    if diag:
        off_diag = ~c.mask.expand(F, Ko, c.M)
        assert torch.equal(_bits(got[off_diag]), _bits(prior[off_diag])), f"{kernel} {case}: an entry off the block diagonals changed"
    if live_kind == "none":
        assert torch.equal(_bits(got), _bits(prior)), f"{kernel} {case}: dead rows added something"
    _check_flow(kernel, case, got, ref, yard, allow)
    if twice:
        again, _, _ = _edge_run(dev, c, live, prior)
        assert torch.equal(_bits(again), _bits(got)), f"{kernel} {case}: a second call is not bit-identical"
    return S


EDGE_B = [1, 2, 33, 64, 65, 129]


@pytest.mark.parametrize("type,H,Ki,Ko", [(R.SUM, 1, 32, 32), (R.SUM, 2, 32, 64), (R.CPT, 2, 64, 64), (R.CPT, 3, 96, 32)])
def test_stats_edge_mfma(hip_device, type, H, Ki, Ko):
    """The matrix-core path: B = 1 (half a row pair), 2, 33 (an odd last pair), 64 | 65 (S = 1 | 2), 129 (S = 3, slices of 44 rows,
    the last with an odd pair); live masks with none, some and all rows dead."""
    for i, B in enumerate(EDGE_B):
        for live_kind in ("some", "all", "none") if B in (2, 33, 129) else ("some",):
            S = _edge_case(hip_device, type, 0, 3, H, Ki, Ko, B, live_kind=live_kind, fold_off=3 if i % 2 else 0, seed=Ki + Ko + B, twice=B == 129)
            assert S == {1: 1, 2: 1, 33: 1, 64: 1, 65: 2, 129: 3}[B]


def test_stats_edge_many_tiles_take_one_slice(hip_device):
    """171 folds of 6 tiles (Ko = 64, sum of 3 x 32 inputs): 1026 tiles >= 1024 force S = 1 at B = 129, an odd last row pair in
    the one slice, no scratch."""
    assert _edge_case(hip_device, R.SUM, 0, 171, 3, 32, 64, 129, seed=5) == 1


@pytest.mark.parametrize("type,diag,H,Ki,Ko", [(R.SUM, 0, 2, 5, 3), (R.SUM, 0, 1, 31, 33), (R.SUM, 0, 1, 32, 33), (R.SUM, 0, 1, 33, 32), (R.SUM, 1, 2, 32, 32),
                                               (R.SUM, 1, 3, 6, 6), (R.CPT, 0, 2, 7, 5), (R.TUCKER, 0, 2, 27, 27), (R.TUCKER, 0, 2, 28, 28), (R.SUM, 0, 1, 1, 1)])
def test_stats_edge_generic(hip_device, type, diag, H, Ki, Ko):
    """The plain path: Ko M = 1023 | 1056 (PC = 1 | 2; 31 x 33 and 32 x 33, 33 x 32), mixing at K = 32 (PC = 2) and 6, Tucker at
    Ki = 27 | 28 (TR = 16 | 8), one unit; B and live masks as above."""
    big = Ki >= 27
    for i, B in enumerate((2, 33, 129) if big else EDGE_B):
        for live_kind in ("some", "all", "none") if B == 33 else ("some",):
            _edge_case(hip_device, type, diag, 2 if big else 3, H, Ki, Ko, B, live_kind=live_kind, fold_off=(2 if big and H == 1 else 3) if i % 2 else 0,
                       seed=Ki + Ko + B, twice=B == 129)


@pytest.mark.parametrize("fam", R.FAMILIES + ["kslow"])
def test_stats_edge_value_families(hip_device, fam):
    """Every value family through both paths; 'kslow' puts e_i + m on both sides of 40: rows that leave the factored product
    (the ballot over the row halves of `stats_edge_mfma`, `ss[r]` of `stats_edge_generic`) next to rows that stay, dead rows
    among them."""
    for type, diag, H, Ki, Ko in ((R.SUM, 0, 2, 32, 32), (R.CPT, 0, 2, 64, 64), (R.SUM, 0, 2, 7, 5), (R.CPT, 0, 2, 7, 5), (R.TUCKER, 0, 2, 6, 5),
                                  (R.SUM, 1, 2, 6, 6)):
        if diag and fam in ("wzero", "kslow"):
            continue
        for B in (33, 129):
            _edge_case(hip_device, type, diag, 2, H, Ki, Ko, B, fam=fam, seed=len(fam) + Ki + B)


# -------------------------------------------------------------------------------------------------------- stats leaves
@pytest.mark.parametrize("x_float", [0, 1])
@pytest.mark.parametrize("K,C", [(5, 3), (32, 256), (64, 256), (300, 40), (75, 256)])
def test_stats_leaf_categorical(hip_device, K, C, x_float):
    """KU = 5 (51 state groups), 32 (8 groups of 32 states), 64 halved to 32 (two blocks), 256 and a block of 44 (one group), 75
    halved to 38 (6 groups of 43 states, a second block of 37 units).
    Sentinels (-1 / NaN and <= -1), an observed state at and beyond C, dead rows; fold_off 2."""
    F, D = 3, 4
    scope = np.array([2, 0, 2], dtype=np.int64)
    for B, fam in BF((1, 33, 130)):
        g = torch.Generator().manual_seed(K + C + B)
        sizes = [7, 9] + [B * K] * F
        off, words = R.arena_offsets(sizes)
        flow = torch.full((words,), NAN)
        for f in range(F):
            R.block(flow, off, 2 + f, B, K).copy_(_leaf_flow(B, K, g, fam))
        ev = torch.randint(-1, C + 2, (B, D), generator=g)
        x = ev
        if x_float:
            x = ev.float() + 0.25 * (ev >= 0)
            x[torch.rand(B, D, generator=g) < 0.1] = NAN
            x[torch.rand(B, D, generator=g) < 0.1] = -1.0
        ntab = torch.softmax(torch.randn(F, K, C, generator=g), -1)
        live = _live(B, "some" if B > 1 else "all", g)
        prior = torch.rand(F, K, C, generator=g)
        fa, _ = _arena(hip_device, sizes, off, flow)
        leaf = _Guarded(F * K * C, hip_device)
        leaf.out.copy_(prior.reshape(-1))
        _status(hip_device, "ck_stats_leaf_categorical", scope, ntab, F, K, C, x, x_float, D, fa.ptr(), np.array(off, dtype=np.int64), 2, live, B,
                leaf.out.data_ptr())
        ref, yard = (R.stats_leaf_categorical(scope, ntab, F, K, C, x, x_float, D, flow, off, 2, live, B, prior, dt) for dt in (F64, F32))
        _check_flow("ck_stats_leaf_categorical", f"K={K} C={C} B={B} x_float={x_float} {fam}", leaf.read().view(F, K, C), ref, yard)
        fa.read([])


@pytest.mark.parametrize("K", [1, 5, 300])
def test_stats_leaf_gaussian(hip_device, K):
    F, D = 3, 3
    scope = np.array([2, 0, 2], dtype=np.int64)
    for B, fam in BF((1, 33, 130)):
        g = torch.Generator().manual_seed(K + B)
        sizes = [5] + [B * K] * F
        off, words = R.arena_offsets(sizes)
        flow = torch.full((words,), NAN)
        for f in range(F):
            R.block(flow, off, 1 + f, B, K).copy_(_leaf_flow(B, K, g, fam))
        x = torch.rand(B, D, generator=g) * 3 + 0.5  # (positive observations: every sum is one of non-negative terms)
        x[torch.rand(B, D, generator=g) < 0.3] = NAN
        mean, std = torch.rand(F, K, generator=g) * 3, torch.exp(torch.rand(F, K, generator=g) * 4 - 3)
        live = _live(B, "some" if B > 1 else "all", g)
        prior = torch.rand(F, K, 3, generator=g)
        fa, _ = _arena(hip_device, sizes, off, flow)
        leaf = _Guarded(F * K * 3, hip_device)
        leaf.out.copy_(prior.reshape(-1))
        _status(hip_device, "ck_stats_leaf_gaussian", scope, mean, std, F, K, x, D, fa.ptr(), np.array(off, dtype=np.int64), 1, live, B, leaf.out.data_ptr())
        ref, yard = (R.stats_leaf_gaussian(scope, mean, std, F, K, x, D, flow, off, 1, live, B, prior, dt) for dt in (F64, F32))
        _check_flow("ck_stats_leaf_gaussian", f"K={K} B={B} {fam}", leaf.read().view(F, K, 3), ref, yard)


def test_stats_unit_sum(hip_device):
    """Folds of Ko = 1, 5, 96, 256 and 300 units in one launch (256 / Ko row groups; above 256 a thread per unit in two steps),
    their sums at shuffled offsets of `unit` with an unused word between them."""
    kos = np.array([1, 5, 96, 256, 300], dtype=np.int32)
    for B, fam in BF((1, 33, 130)):
        g = torch.Generator().manual_seed(B)
        sizes = [B * int(k) for k in kos]
        off, words = R.arena_offsets(sizes)
        flow = torch.full((words,), NAN)
        for f, k in enumerate(kos):
            R.block(flow, off, f, B, int(k)).copy_(_leaf_flow(B, int(k), g, fam))
        unit_off = np.array([661, 0, 6, 404, 103], dtype=np.int64)  # (a free word between any two folds)
        n = 664
        live = _live(B, "some" if B > 1 else "all", g)
        prior = torch.rand(n, generator=g)
        fa, _ = _arena(hip_device, sizes, off, flow)
        unit = _Guarded(n, hip_device)
        unit.out.copy_(prior)
        _status(hip_device, "ck_stats_unit_sum", fa.ptr(), np.array(off, dtype=np.int64), kos, unit_off, 5, live, B, unit.out.data_ptr())
        ref, yard = (R.stats_unit_sum(flow, off, kos, unit_off, 5, live, B, prior, dt) for dt in (F64, F32))
        got = unit.read()
        own = torch.zeros(n, dtype=torch.bool)
        for o, k in zip(unit_off, kos):
            own[int(o):int(o) + int(k)] = True
        assert torch.equal(_bits(got[~own]), _bits(prior[~own])), "a word of `unit` outside every fold changed"
        _check_flow("ck_stats_unit_sum", f"B={B} {fam}", got, ref, yard)
