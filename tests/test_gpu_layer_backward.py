"""The layer-wise backward of the real lse-sum semiring (cirkit_amd/csrc/ck_backward.hip), kernel by kernel: `ck_sum_lse_bwd`,
`ck_mixing_lse_bwd`, `ck_categorical_bwd`, `ck_gaussian_bwd`, `ck_hadamard_bwd`, `ck_kronecker_bwd`, `ck_segment_add_rows` through
the C ABI on raw buffers against the fp64 run of tests/layer_backward_restatement.py (pinned to torch autograd by
tests/test_layer_backward_restatement.py), on both sides of every boundary of the host dispatch and of the kernels it picks.

The shapes are read off the dispatch at this commit (line numbers of ck_backward.hip; nothing asserts which kernel ran):
* `ck_sum_lse_bwd` (1489-1569): `sum_lse_bwd_scalar32` for Ki = 32, Ko = 1, PROD or H = 1 (1498-1503: 256 rows per block of 32
  half-waves); `sum_lse_bwd_tile32` / `tile64` for Ki = Ko = 32 / 64, PROD or H = 1, all four buffers 16-byte aligned (1504-1533),
  with tiles_per_wave doubled up to 8 while 8 tpw tiles fit the batch and F ceil(tiles / (8 tpw)) >= 2048 (K = 64: 1024) (1509-1511,
  1519-1521); else `sum_lse_bwd_generic<TB>` with TB = 16 halved down to 4 while the LDS need exceeds 64 KB, and 1 for a KRON layer
  above 160 KB (1541-1548).  `ck_debug_force_generic_bwd(1)` sends everything to the generic kernel.
* `ck_mixing_lse_bwd` (1407-1431): `mixing_bwd_reg_kernel<4|8|16>` for K = 32 / 64 and H <= 16, rows_per_block 16 doubled up to 512
  while F ceil(B / (2 rpb)) >= 2048 (1417-1425); else the LDS-atomic `mixing_bwd_kernel`, 64 rows per block (1427-1430).
* `ck_categorical_bwd` (1599-1634): the sorted kernel for K % 32 == 0, B >= 256 and (C + 1) K + 2 C + 3 + 4096 words of LDS within
  160 KB (1605-1606), rows sorted 4096 at a time; else the unsorted one (float4 per lane for K % 4 == 0, from 643); dynamic LDS
  above 48 KB needs the attribute (1610, 1625).
* `ck_segment_add_rows` (1478-1487): float4 for block_elems % 4 == 0; per child ceil(work / 256) blocks of 256 threads, at most
  4096, with work counted in float4s on that path and in words on the scalar one (1484-1485).
* `ck_gaussian_bwd` (1397-1405): one workgroup per fold, min(K, 256) units x 256 / that row groups.

Memory.  The gradient arena is ONE allocation of child blocks between guard words of a NaN bit pattern no kernel produces
(`_GuardedArena`); with accumulate = 0 every word of every targeted block must be written and every other word keep the pattern;
with accumulate = 1 / 2 every block carries a random prior and every word outside the targeted blocks must come back bit for bit.
dW / dmw always carry a random prior (the header says "+="), dtable with accumulate = 1; dmean / dstddev / dtable with
accumulate = 0 must be written entirely.  Every row_off is a multiple of 4 words.

Tolerance (the convention of tests/test_gpu_param_backward.py).  The yardstick of a case is the error of the SAME restated function
run in fp32 by torch on the CPU against its fp64 run on the case's own inputs, the accumulate step included; the GPU must be within
4 x that, with a floor of 1e-6.  Errors are relative to max|row| of the fp64 result (garena: the units of one batch row of one
block; parameter gradients: the last axis).  Nothing in a bar comes from what the GPU returns, no entry is left out, a non-finite
reference entry must be matched exactly.  Derived bounds: a destination that receives m addends in an order the launch does not
fix (dW and dmw: m = B; garena under accumulate = 2: m = the (fold, child) pairs that target the word; dtable: m = the rows that
select the category) may additionally be off by m 2^-24 (|prior| + sum|addends|), the bound of `ck_param_scatter_add_folds`;
`ck_hadamard_bwd` with accumulate = 0 is a copy: bit equality; `ck_segment_add_rows` adds in list order, one fp32 rounding per
addition: bit equality with the fp32 run of its restatement.

Rounding allowance of the sum layers and the Gaussian (measured first without: LAB_NOTES.md, "Layer backward").  gv_n = e_n sum_o
W[o, n] gout_o / y_o sums terms of both signs, and max|row| of a row that cancellation leaves small compares two single draws of
amplified rounding noise: 4 of 2391 cases of `ck_sum_lse_bwd` stood between 4.0 and 6.3 x their yardstick, three of them in the
generic kernel (plain expf, fmaf, IEEE division).  So an entry may additionally be off by the first-order bound of ANY fp32
evaluation, from the fp64 terms of the case alone (u = 2^-24):
* e_n = exp(v_n - m): the rounded difference and its rounded product with log2 e move the argument by at most 2 u |v_n - m| log2 e,
  i.e. e_n by 2 u |v_n - m| relative; v_exp_f32 and expf are good to one ulp = 2 u.  eps_n = 2 u (1 + |v_n - m|).
* y_o = sum_n W e_n, all terms >= 0: the eps_n weighted by the terms, plus N u of summation in any order.  v_rcp_f32 one ulp (2 u),
  the product with gout u: gy_o is within kappa_o = (sum_n W e_n eps_n) / y_o + (N + 3) u, relative.
* sum_o W[o, n] gy_o: Ko u of summation on the sum of the |terms|; the product with e_n: u and eps_n.  A KRON child's unit sums
  N / Ki such entries: N / Ki more u.
  allowance(gv_n) = e_n sum_o W[o, n] |gy_o| (kappa_o + (Ko + 1 [+ N / Ki]) u) + eps_n e_n sum_o W[o, n] |gy_o|,
  and the same per addend gy_o e_n of dW (on top of the m 2^-24 term above for their order).
`ck_gaussian_bwd`: an addend gout (x - mu) / sd^2 or gout ((x - mu)^2 / sd^3 - 1 / sd) carries at most 8 roundings on
|gout| |x - mu| / sd^2 or |gout| ((x - mu)^2 / sd^3 + 1 / sd) and the B addends are summed in the kernel's order, not torch's
(1025-1047): a thread adds the rows of its group, every `groups`-th with groups = 256 / min(K, 256), one rounding per fmaf, and one
thread then adds the groups' partial sums in turn (a group without rows holds 0, which adds exactly).  An addend meets at most
ceil(B / groups) + min(groups, B) roundings of summation: (ceil(B / groups) + min(groups, B) + 8) u times the sum of those
magnitudes -- 268 u at K = 1, B = 1000, 79 u at K = 5, and (B + 9) u only from K = 256, where one thread adds all the rows of a unit
(K = 1, B = 256 stood at 4.6 x, K = 300, B = 1000 at 4.5 x).
The 4 x bar stands for everything else, and for these on top of the allowance.  Every case prints `LAYER-BWD <kernel> <case> err yard ratio`
(ratio = err / max(yard, floor / 4): a case passes iff ratio <= 4); the worst per kernel are in LAB_NOTES.md, "Layer backward"."""
import contextlib

import numpy as np
import pytest
import torch

import layer_backward_restatement as R
from guarded_buffers import NAN_BITS, NEG_INF, _Guarded, _GuardedArena, _logits, _stream

pytestmark = pytest.mark.gpu

FLOOR = 1e-6
EPS = 2.0 ** -24
WORST: dict[str, tuple] = {}
CASES = [0]
FAMILIES = ["normal", "shift", "spread", "neginf", "infrows", "wzero", "gzero"]


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for kernel in sorted(WORST):
        r, case, err, yard = WORST[kernel]
        print(f"\nLAYER-BWD-WORST {kernel}: ratio {r:.3f} (err {err:.3e}, yardstick {yard:.3e}) at {case}")
    print(f"\nLAYER-BWD-CASES {CASES[0]}")


def _call(dev, name, *args):
    """The entry point on the current stream, then a synchronize.  A host tensor among `args` is copied to the device and kept
    alive until the launch has finished; its pointer is what the entry point receives."""
    from cirkit_amd import _capi as capi

    held = [a.contiguous().to(dev) if isinstance(a, torch.Tensor) else a for a in args]
    capi.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in held], _stream(dev))
    torch.cuda.synchronize()


@contextlib.contextmanager
def _forced_generic(on):
    from cirkit_amd import _capi as capi

    if on:
        capi.call("ck_debug_force_generic_bwd", 1)
    try:
        yield
    finally:
        if on:
            capi.call("ck_debug_force_generic_bwd", 0)


def _report(kernel, case, err, yard):
    err, yard = float(err), float(yard)
    ratio = err / max(yard, FLOOR / 4)
    print(f"LAYER-BWD {kernel} {case} err {err:.3e} yard {yard:.3e} ratio {ratio:.3f}")
    CASES[0] += 1
    if kernel not in WORST or ratio > WORST[kernel][0]:
        WORST[kernel] = (ratio, case, err, yard)
    assert err <= max(4 * yard, FLOOR), f"{kernel} {case}: error {err:.3e} above 4 x the fp32 yardstick {yard:.3e} (floor {FLOOR})"


def _row_scale(ref):
    """max|row| of the fp64 result along the last axis over its finite entries (1 where that is 0: the error is then absolute)."""
    a = torch.where(torch.isfinite(ref), ref.abs(), torch.zeros_like(ref)).amax(dim=-1, keepdim=True)
    return torch.where(a > 0, a, torch.ones_like(a))


def _check(kernel, case, got, ref, yard, extra=None):
    """got (fp32, from the GPU) against ref (fp64) with the fp32 yardstick run `yard`, relative to max|row| of ref; `extra`
    (fp64, from the inputs alone): the derived allowance of an entry, taken off its error first.  Non-finite reference entries
    are matched exactly; every other entry is compared."""
    got, yard = got.double().reshape(ref.shape), yard.double().reshape(ref.shape)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{kernel} {case}: NaN where the reference has none (or the reverse)"
    if not bool(fin.all()):
        inf = torch.isinf(ref)
        assert torch.equal(got[inf], ref[inf]), f"{kernel} {case}: an infinite reference entry is not matched"
    assert bool((torch.isfinite(got) | ~fin).all()), f"{kernel} {case}: non-finite where the reference is finite"
    assert bool((torch.isfinite(yard) | ~fin).all()), f"{kernel} {case}: the fp32 yardstick run is not finite where the fp64 run is"
    s = _row_scale(ref)
    d = (got - ref).abs()
    if extra is not None:
        d = (d - extra.reshape(ref.shape)).clamp_(min=0)
    zero = torch.zeros((), dtype=torch.float64)
    _report(kernel, case, torch.where(fin, d / s, zero).max(), torch.where(fin, (yard - ref).abs() / s, zero).max())


# ------------------------------------------------------------------------------------------------------- shared pieces
def _blocks(n_blocks, B, K, fam, g):
    """(n_blocks, B, K) fp32 activations of a value family: randn * 2; 'shift': the same 4000 nats down (the magnitude the
    kernel comment at ck_backward.hip:122-124 is about); 'spread': uniform over +-100 (e underflows); 'neginf': about 30 % of
    the units -inf; 'infrows': rows 0 and B // 2 -inf in every block.

    'spread+anchor' is the spread of the mixing layer: uniform over [-200, 0] with, at every (row, unit), the blocks of one
    parity within randn of 0 (neighbouring blocks -- the children of a fold -- have both parities).  e of the other children
    underflows (to subnormals and to 0) while y[k] stays a normal number.  A unit whose children ALL lie 87 to 103 nats below the
    row's maximum has a subnormal y[k] in fp32; gout / y overflows and inf * 0 follows, in torch's fp32 autograd through the
    reference's forward as in any fp32 evaluation with one maximum per row: there is no fp32 yardstick for it."""
    if fam == "spread+anchor":
        x = torch.rand((n_blocks, B, K), generator=g) * -200.0
        i, b, k = torch.meshgrid(torch.arange(n_blocks), torch.arange(B), torch.arange(K), indexing="ij")
        return torch.where((i + b + k) % 2 == 0, torch.randn((n_blocks, B, K), generator=g), x)
    if fam == "spread":
        return _logits((n_blocks, B, K), "spread", g)
    if fam == "neginf":
        return _logits((n_blocks, B, K), "neginf", g) * 2
    x = _logits((n_blocks, B, K), "normal", g) * 2
    if fam == "shift":
        x = x - 4000.0
    if fam == "infrows":
        x[:, 0] = NEG_INF
        x[:, B // 2] = NEG_INF
    return x


def _weights(shape, fam, g):
    """Positive rows summing to 1 over the last axis; 'wzero': the last column 0 (a padded plan's), row 0 of the middle axis 0 when
    there is more than one, and 10 % of the entries exactly 0."""
    w = torch.softmax(torch.randn(shape, generator=g), -1)
    if fam == "wzero":
        w[torch.rand(shape, generator=g) < 0.1] = 0.0
        if shape[-1] > 1:
            w[..., -1] = 0.0
        if shape[-2] > 1:
            w[..., 0, :] = 0.0
    return w.contiguous()


def _gout(F, B, Ko, fam, g):
    """randn; 'gzero': 20 % exact zeros and row B // 3 zero; 'infrows': row 0 zero (row B // 2, the other -inf row, is not)."""
    go = torch.randn(F, B, Ko, generator=g)
    if fam == "gzero":
        go[torch.rand(F, B, Ko, generator=g) < 0.2] = 0.0
        go[:, B // 3] = 0.0
    if fam == "infrows":
        go[:, 0] = 0.0
    return go


class _Layer:
    """The arenas of one launch of a layer with H children per fold, blocks of B x K words: the input arena (`share` > 0: the
    folds draw their children from that many blocks, (f + h) % share; else one block per (fold, child)) and the gradient arena by
    `grad`: 'mirror' (grad_row_off NULL: the input arena's own offsets), 'distinct' (one block per (fold, child) in shuffled
    order, and one more nobody targets), 'one' (every (fold, child) targets block 0 of two).  `twice`: child 1 of every fold is
    its child 0 again."""

    def __init__(self, dev, F, H, B, K, acc, grad, share, fam, g, lead=0, twice=False):
        self.dev, self.F, self.H, self.B, self.K, self.acc, self.n, self.g = dev, F, H, B, K, acc, B * K, g
        n_in = share if share else F * H
        self.arena_dev = _GuardedArena([self.n] * n_in, dev, lead)
        self.arena = self.arena_dev.fill(list(_blocks(n_in, B, K, fam, g)))  # (host, fp32, NaN between the blocks)
        pick = np.array([[(f + h) % share if share else f * H + h for h in range(H)] for f in range(F)])
        if twice:
            pick[:, 1] = pick[:, 0]
        off = np.array(self.arena_dev.off, dtype=np.int64)
        self.row_off = off[pick]
        self.n_g = {"mirror": n_in, "distinct": F * H + 1, "one": 2}[grad]
        self.lead = lead
        if grad == "mirror":
            self.tpick, self.grow = pick, None
        elif grad == "distinct":
            self.tpick = torch.randperm(F * H, generator=g).numpy().reshape(F, H)
        else:
            self.tpick = np.zeros((F, H), dtype=np.int64)
        self.targets = sorted(set(int(t) for t in self.tpick.reshape(-1)))
        self.new_garena()
        self.goff = np.array(self.garena.off, dtype=np.int64)[self.tpick]
        if grad != "mirror":
            self.grow = self.goff
        assert bool((self.row_off % 4 == 0).all()) and bool((self.goff % 4 == 0).all())

    def new_garena(self):
        """A fresh gradient arena (with the SAME prior as before, when the kernel is to add)."""
        self.garena = _GuardedArena([self.n] * self.n_g, self.dev, self.lead)
        if self.acc:
            if not hasattr(self, "_prior"):
                self._prior = [torch.randn(self.n, generator=self.g) for _ in range(self.n_g)]
            self.prior = self.garena.fill(self._prior)
        else:
            self.prior = torch.full((self.garena.words,), NAN_BITS, dtype=torch.int32).view(torch.float32)

    def ptrs(self):
        """(arena, garena, row_off, grad_row_off) as the entry points take them."""
        return (self.arena_dev.ptr(), self.garena.ptr(), torch.from_numpy(self.row_off),
                None if self.grow is None else torch.from_numpy(self.grow))

    def blocks_of(self, flat):
        """(targets, B, K) of a flat arena."""
        if not hasattr(self, "_idx"):
            o = torch.as_tensor(np.array(self.garena.off, dtype=np.int64)[self.targets])
            self._idx = o.unsqueeze(-1) + torch.arange(self.n)
        return flat[self._idx].view(len(self.targets), self.B, self.K)

    def check_garena(self, kernel, case, ref, yard, G64, allow=None):
        """The targeted blocks of the GPU's gradient arena against the restated one; G64: the fp64 gradients (F, H, B, K) (for
        the bound of accumulate = 2); allow (F, H, B, K): a derived allowance of every (fold, child) gradient."""
        got = self.garena.read(self.targets)
        extra = None
        zero = torch.zeros(self.garena.words, dtype=torch.float64)
        if self.acc == 2:
            ones = torch.ones(self.F, self.H, self.B, self.K, dtype=torch.float64)
            m = R.scatter_children(zero, self.goff, ones, 2)
            mass = R.scatter_children(torch.nan_to_num(self.prior.double()).abs(), self.goff, G64.abs(), 2)
            extra = self.blocks_of(m * EPS * mass)
        if allow is not None:
            a = self.blocks_of(R.scatter_children(zero, self.goff, allow, 2))
            extra = a if extra is None else extra + a
        ref_b = self.blocks_of(ref)
        _check(kernel, case, self.blocks_of(got), ref_b, self.blocks_of(yard), extra)
        return self.blocks_of(got), ref_b


def _dw_check(kernel, case, buf, shape, ref, yard, prior, addends_mass, m, allow=None):
    """dW / dmw: m addends in any order on top of the prior (`allow`: a derived allowance on top)."""
    extra = m * EPS * (prior.double().abs() + addends_mass)
    if allow is not None:
        extra = extra + allow
    _check(kernel, case, buf.read().view(shape), ref, yard, extra)


# ------------------------------------------------------------------------------------------------------ ck_sum_lse_bwd
def _sum_rounding_allowance(L, w64, gout64, terms, Ki, Ko, mode):
    """(F, H, B, Ki), (F, Ko, N): what fp32 rounding can do to the children gradients and to the addends of dW in ANY evaluation
    of gv_n = e_n sum_o W[o, n] gout_o / y_o with a one-ulp exponential and a one-ulp reciprocal, to first order in u = 2^-24
    (the derivation is in the module docstring).  From the fp64 terms of the case alone."""
    e, gy = terms
    pos = e > 0
    below = torch.where(pos, -torch.log(torch.where(pos, e, torch.ones_like(e))), torch.zeros_like(e))  # |v_n - m| (KRON: summed over the children)
    eps_e = 2 * EPS * (1 + below)
    y = torch.einsum("fon,fbn->fbo", w64, e)
    eps_y = torch.where(y > 0, torch.einsum("fon,fbn->fbo", w64, e * eps_e) / torch.where(y > 0, y, torch.ones_like(y)), torch.zeros_like(y))
    N = e.shape[-1]
    c = N + Ko + 4 + (N // Ki if mode == R.KRON else 0)
    args = (L.arena.double(), L.row_off, w64, gout64, L.B, Ki, mode)
    G1, dW1 = R.sum_lse_grads(*args, (e, gy.abs() * (eps_y + c * EPS)))
    G2, dW2 = R.sum_lse_grads(*args, (e * eps_e, gy.abs()))
    return G1 + G2, dW1 + dW2


def _sum_case(dev, kernel, case, *, F, H, B, Ki, Ko, mode, acc, grad="mirror", share=0, fam="normal", lead=0, twice=False, seed=0,
              forced=(False,)):
    from cirkit_amd import _capi as capi

    g = torch.Generator().manual_seed(seed)
    N = Ki if mode == R.PROD else (H * Ki if mode == R.CAT else Ki ** H)
    L = _Layer(dev, F, H, B, Ki, acc, grad, share, fam, g, lead, twice)
    w, gout, dw_prior = _weights((F, Ko, N), fam, g), _gout(F, B, Ko, fam, g), torch.randn(F, Ko, N, generator=g)
    unused_out = torch.full((16,), float("nan"))  # (`out` must not be NULL and is not read: y is recomputed)
    terms = R.sum_lse_terms(L.arena.double(), L.row_off, w.double(), gout.double(), B, Ki, mode)
    G64, dW64 = R.sum_lse_grads(L.arena.double(), L.row_off, w.double(), gout.double(), B, Ki, mode, terms)
    ref_g, ref_dw = R.scatter_children(L.prior.double(), L.goff, G64, acc), dw_prior.double() + dW64
    G32, dW32 = R.sum_lse_grads(L.arena, L.row_off, w, gout, B, Ki, mode)
    yard_g, yard_dw = R.scatter_children(L.prior, L.goff, G32, acc), dw_prior + dW32
    dw_mass = torch.einsum("fbo,fbn->fon", terms[1].abs(), terms[0])
    Gx, dWx = _sum_rounding_allowance(L, w.double(), gout.double(), terms, Ki, Ko, mode)
    del terms, G32, dW32
    wd, gd = w.to(dev), gout.to(dev)
    code = {R.CAT: capi.CK_SUM_CAT, R.PROD: capi.CK_SUM_PROD, R.KRON: capi.CK_SUM_KRON}[mode]
    for force in forced:
        if force:
            L.new_garena()
        dw = _Guarded(F * Ko * N, dev)
        dw.out.copy_(dw_prior.reshape(-1))
        with _forced_generic(force):
            _call(dev, "ck_sum_lse_bwd", *L.ptrs(), wd.data_ptr(), unused_out, gd.data_ptr(), dw.out.data_ptr(), F, H, B, Ki, Ko, code, acc)
        k = "sum:generic(forced)" if force else kernel
        got_b, ref_b = L.check_garena(k + ":garena", case, ref_g, yard_g, G64, Gx)
        if acc == 0:
            assert bool((got_b[ref_b == 0] == 0).all()), f"{k} {case}: a gradient that is exactly 0 (a -inf input, a zero gout or weight) is not"
        _dw_check(k + ":dW", case, dw, (F, Ko, N), ref_dw, yard_dw, dw_prior, dw_mass, B, dWx)


def _grads_and_modes(cases):
    """Every case once with grad_row_off NULL and once distinct, accumulate cycling through 0 / 1 / 2."""
    i = 0
    for c in cases:
        for grad in ("mirror", "distinct"):
            yield c, grad, i % 3
            i += 1


SCALAR_LAYERS = [(R.PROD, 1), (R.PROD, 2), (R.PROD, 3), (R.CAT, 1)]
MODE_NAME = {R.CAT: "CAT", R.PROD: "PROD", R.KRON: "KRON"}


@pytest.mark.parametrize("B", [1, 31, 255, 256, 257, 600])
def test_sum_scalar32(hip_device, B):
    """Ki = 32, Ko = 1: a half-wave per row, 32 of them per block of 256 rows -- one row, less than the half-waves, both sides
    of a block, three blocks with a ragged last; then the generic kernel on the same cases."""
    for (mode, H), grad, acc in _grads_and_modes(SCALAR_LAYERS):
        _sum_case(hip_device, "sum:scalar32", f"{MODE_NAME[mode]} H={H} B={B} grad={grad} acc={acc}", F=3, H=H, B=B, Ki=32, Ko=1, mode=mode,
                  acc=acc, grad=grad, seed=B + H, forced=(False, True))


@pytest.mark.parametrize("B", [1, 31, 32, 33, 127, 128, 129, 257])
@pytest.mark.parametrize("K", [32, 64])
def test_sum_tile(hip_device, K, B):
    """Ki = Ko = 32 / 64 at F = 3 (tiles_per_wave = 1): less than a tile, both sides of one tile, of the four tiles of a
    workgroup and of two workgroups; PROD with 1 .. 3 children and CAT with one; then the generic kernel on the same cases."""
    for (mode, H), grad, acc in _grads_and_modes(SCALAR_LAYERS):
        _sum_case(hip_device, f"sum:tile{K}", f"{MODE_NAME[mode]} H={H} B={B} grad={grad} acc={acc}", F=3, H=H, B=B, Ki=K, Ko=K, mode=mode,
                  acc=acc, grad=grad, seed=K + B + H, forced=(False, True))


@pytest.mark.parametrize("K,F,B,H,grad,acc", [(32, 1024, 500, 2, "distinct", 0), (32, 1024, 1057, 1, "distinct", 0), (64, 512, 1057, 1, "distinct", 0),
                                              (32, 1024, 500, 2, "one", 2)])
def test_sum_tile_many_folds(hip_device, K, F, B, H, grad, acc):
    """tiles_per_wave above 1 (ck_backward.hip:1509-1511, 1519-1521): F = 1024, B = 500 gives 2 at K = 32; F = 1024, B = 1057
    gives 8, with a wave whose second tile holds one row and whose later tiles lie beyond B; F = 512, B = 1057 gives 8 at
    K = 64.  The folds read three shared input blocks and write a block each; in the last case all of them add into one."""
    _sum_case(hip_device, f"sum:tile{K}", f"PROD F={F} H={H} B={B} grad={grad} acc={acc}", F=F, H=H, B=B, Ki=K, Ko=K, mode=R.PROD, acc=acc,
              grad=grad, share=3, seed=F + B, forced=(False, True))


@pytest.mark.parametrize("K", [32, 64])
def test_sum_leaves_the_tile_path(hip_device, K):
    """CAT with two children (N = 2 K) and an arena whose base is 4 bytes off 16-byte alignment (the `aligned16` checks,
    ck_backward.hip:1504-1505, 1516-1517) go to the generic kernel."""
    for acc in (0, 1):
        _sum_case(hip_device, "sum:generic", f"CAT H=2 K={K} B=33 acc={acc}", F=3, H=2, B=33, Ki=K, Ko=K, mode=R.CAT, acc=acc, seed=K)
        _sum_case(hip_device, "sum:generic", f"PROD H=2 K={K} B=33 base+4 acc={acc}", F=3, H=2, B=33, Ki=K, Ko=K, mode=R.PROD, acc=acc, lead=1,
                  seed=K + 1)
        _sum_case(hip_device, "sum:generic", f"PROD H=2 K={K} B=33 base+4 distinct acc={acc}", F=3, H=2, B=33, Ki=K, Ko=K, mode=R.PROD, acc=acc,
                  grad="distinct", lead=1, seed=K + 2)


@pytest.mark.parametrize("Ki,Ko", [(1, 1), (5, 3), (33, 32), (64, 32), (32, 64), (7, 65), (6, 130)])
def test_sum_generic(hip_device, Ki, Ko):
    """N on both sides of the 32-wide chunk of W and Ko of the 64-wide one; B on both sides of the 16-row tile."""
    cases = [(mode, H, B) for mode in (R.CAT, R.PROD) for H in (1, 2, 3) for B in (1, 15, 16, 17, 40)]
    for (mode, H, B), grad, acc in _grads_and_modes(cases):
        _sum_case(hip_device, "sum:generic", f"{MODE_NAME[mode]} Ki={Ki} Ko={Ko} H={H} B={B} grad={grad} acc={acc}", F=3, H=H, B=B, Ki=Ki, Ko=Ko,
                  mode=mode, acc=acc, grad=grad, seed=Ki + Ko + H + B)


@pytest.mark.parametrize("mode,H,Ki,Ko", [(R.CAT, 8, 64, 5), (R.CAT, 16, 64, 5), (R.KRON, 2, 3, 5), (R.KRON, 2, 8, 5), (R.KRON, 2, 64, 5),
                                          (R.KRON, 3, 4, 5), (R.KRON, 2, 72, 8)])
def test_sum_generic_by_lds_budget(hip_device, mode, H, Ki, Ko):
    """TB by the LDS need (ck_backward.hip:1541-1548): CAT N = 512 gives 8, N = 1024 gives 4; KRON N = 4096 stays at 4 above
    48 KB, N = 5184 gives 1; small KRON layers 16."""
    for grad, acc in (("mirror", 0), ("distinct", 1), ("mirror", 2)):
        for B in ((3,) if Ki >= 64 else (3, 17)):
            _sum_case(hip_device, "sum:generic", f"{MODE_NAME[mode]} Ki={Ki} Ko={Ko} H={H} B={B} grad={grad} acc={acc}", F=2, H=H, B=B, Ki=Ki, Ko=Ko,
                      mode=mode, acc=acc, grad=grad, seed=H + Ki)


def test_sum_children_shared_within_the_layer(hip_device):
    """accumulate = 2: a CAT fold that names the same child twice, folds that share children, and all into one block."""
    for mode, H, Ki, Ko in ((R.CAT, 2, 5, 3), (R.PROD, 2, 32, 32), (R.KRON, 2, 3, 4), (R.PROD, 3, 32, 1)):
        _sum_case(hip_device, "sum:shared", f"{MODE_NAME[mode]} Ki={Ki} Ko={Ko} child twice", F=3, H=H, B=17, Ki=Ki, Ko=Ko, mode=mode, acc=2, twice=True,
                  seed=Ki)
        _sum_case(hip_device, "sum:shared", f"{MODE_NAME[mode]} Ki={Ki} Ko={Ko} 5 folds on 3 blocks", F=5, H=H, B=17, Ki=Ki, Ko=Ko, mode=mode, acc=2,
                  share=3, seed=Ki + 1)
        _sum_case(hip_device, "sum:shared", f"{MODE_NAME[mode]} Ki={Ki} Ko={Ko} all into one block", F=5, H=H, B=17, Ki=Ki, Ko=Ko, mode=mode, acc=2,
                  share=3, grad="one", seed=Ki + 2)


@pytest.mark.parametrize("fam", FAMILIES)
def test_sum_value_families(hip_device, fam):
    """Every value family through every kernel (and the generic one on the MFMA shapes): B = 33 is a full tile and a ragged one,
    two blocks of the generic kernel and a ragged third."""
    shapes = [("sum:scalar32", R.PROD, 2, 32, 1, True), ("sum:tile32", R.PROD, 2, 32, 32, True), ("sum:tile64", R.PROD, 2, 64, 64, True),
              ("sum:tile32", R.CAT, 1, 32, 32, True), ("sum:generic", R.CAT, 2, 5, 3, False), ("sum:generic", R.PROD, 2, 33, 32, False),
              ("sum:generic", R.KRON, 2, 3, 4, False)]
    for kernel, mode, H, Ki, Ko, mfma in shapes:
        for acc in (0, 1):
            _sum_case(hip_device, kernel, f"{MODE_NAME[mode]} Ki={Ki} Ko={Ko} H={H} B=33 {fam} acc={acc}", F=2, H=H, B=33, Ki=Ki, Ko=Ko, mode=mode,
                      acc=acc, fam=fam, seed=len(fam) + Ki, forced=(False, True) if mfma else (False,))


# --------------------------------------------------------------------------------------------------- ck_mixing_lse_bwd
def _mixing_case(dev, kernel, case, *, F, H, B, K, acc, grad="mirror", share=0, fam="normal", seed=0):
    g = torch.Generator().manual_seed(seed)
    L = _Layer(dev, F, H, B, K, acc, grad, share, "spread+anchor" if fam == "spread" else fam, g)
    mw, gout, d_prior = _weights((F, K, H), fam, g), _gout(F, B, K, fam, g), torch.randn(F, K, H, generator=g)
    terms = R.mixing_lse_terms(L.arena.double(), L.row_off, mw.double(), gout.double(), B, K)
    G64, d64 = R.mixing_lse_grads(L.arena.double(), L.row_off, mw.double(), gout.double(), B, K)
    G32, d32 = R.mixing_lse_grads(L.arena, L.row_off, mw, gout, B, K)
    ref_g, yard_g = R.scatter_children(L.prior.double(), L.goff, G64, acc), R.scatter_children(L.prior, L.goff, G32, acc)
    mass = (terms[1].abs().unsqueeze(1) * terms[0]).sum(2).permute(0, 2, 1)
    dmw = _Guarded(F * K * H, dev)
    dmw.out.copy_(d_prior.reshape(-1))
    _call(dev, "ck_mixing_lse_bwd", *L.ptrs(), mw, gout, dmw.out.data_ptr(), F, H, B, K, acc)
    got_b, ref_b = L.check_garena(kernel + ":garena", case, ref_g, yard_g, G64)
    if acc == 0:
        assert bool((got_b[ref_b == 0] == 0).all()), f"{kernel} {case}: a gradient that is exactly 0 (a -inf row, a zero gout or coefficient) is not"
    _dw_check(kernel + ":dmw", case, dmw, (F, K, H), d_prior.double() + d64, d_prior + d32, d_prior, mass, B)


MIX_B = [1, 15, 16, 17, 33, 63, 64, 65, 200]


@pytest.mark.parametrize("H", [1, 2, 4, 5, 8, 9, 16])
@pytest.mark.parametrize("K", [32, 64])
def test_mixing_register_kernels(hip_device, K, H):
    """K = 32 / 64, H on both sides of the 4 / 8 / 16 register files; B on both sides of the 16 rows of a workgroup (F = 2:
    rows_per_block 16) and of the 64 / K rows of a wave pass."""
    for B, grad, acc in _grads_and_modes(MIX_B):
        _mixing_case(hip_device, "mixing:reg", f"K={K} H={H} B={B} grad={grad} acc={acc}", F=2, H=H, B=B, K=K, acc=acc, grad=grad, seed=K + H + B)


@pytest.mark.parametrize("K,H", [(1, 2), (6, 2), (24, 2), (33, 2), (128, 2), (1, 3), (6, 3), (24, 3), (33, 3), (128, 3), (32, 17)])
def test_mixing_lds_kernel(hip_device, K, H):
    """Every other shape: K below, at and above a wave's 64 lanes; 64 rows per block, four waves striding them."""
    for B, grad, acc in _grads_and_modes(MIX_B):
        _mixing_case(hip_device, "mixing:lds", f"K={K} H={H} B={B} grad={grad} acc={acc}", F=2, H=H, B=B, K=K, acc=acc, grad=grad, seed=K + H + B)


@pytest.mark.parametrize("grad,acc", [("distinct", 0), ("distinct", 1), ("one", 2), ("mirror", 2)])
def test_mixing_many_folds(hip_device, grad, acc):
    """F = 2048, B = 70 at K = 32, H = 2: rows_per_block 512 > B (ck_backward.hip:1417-1419); the folds read three shared blocks."""
    _mixing_case(hip_device, "mixing:reg", f"F=2048 K=32 H=2 B=70 grad={grad} acc={acc}", F=2048, H=2, B=70, K=32, acc=acc, grad=grad, share=3, seed=7)


@pytest.mark.parametrize("fam", FAMILIES)
def test_mixing_value_families(hip_device, fam):
    """'infrows' is the case of the header's guard: rows 0 and B // 2 have every input -inf (y = 0), the first with gout = 0 and
    the second with gout != 0 -- 0 in garena for both, dmw untouched by them (the parent kernels returned NaN in the rows and in
    the whole dmw of the fold).  'wzero' holds coefficients that are exactly 0.  'spread' is the anchored one of `_blocks` (blocks
    of their own for every (fold, child): the anchors go by block parity)."""
    for kernel, K, H in (("mixing:reg", 32, 2), ("mixing:reg", 64, 5), ("mixing:lds", 6, 3), ("mixing:lds", 128, 2)):
        for acc in (0, 1, 2):
            _mixing_case(hip_device, kernel, f"K={K} H={H} B=33 {fam} acc={acc}", F=2, H=H, B=33, K=K, acc=acc, fam=fam, seed=len(fam) + K,
                         share=3 if acc == 2 and fam != "spread" else 0)


# -------------------------------------------------------------------------------- ck_hadamard_bwd / ck_kronecker_bwd
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("H", [1, 2, 3, 16])
def test_hadamard(hip_device, H, B):
    """Every child receives gout: with accumulate = 0 bit for bit; 1 on a prior; 2 with children shared between the folds."""
    for K in (5, 32):
        for acc in (0, 1, 2):
            g = torch.Generator().manual_seed(H + B + K)
            F = 4
            L = _Layer(hip_device, F, H, B, K, acc, "mirror", 3 if acc == 2 else 0, "normal", g)
            gout = torch.randn(F, B, K, generator=g)
            _call(hip_device, "ck_hadamard_bwd", L.garena.ptr(), torch.from_numpy(L.row_off), gout, F, H, B, K, acc)
            G = gout.unsqueeze(1).expand(F, H, B, K)
            got_b, _ = L.check_garena("hadamard", f"H={H} B={B} K={K} acc={acc}", R.hadamard_bwd(L.prior.double(), L.row_off, gout.double(), H, acc),
                                      R.hadamard_bwd(L.prior, L.row_off, gout, H, acc), G.double())
            if acc == 0:
                assert torch.equal(got_b.view(F, H, B, K), G), "not a copy of gout"


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("H,K", [(2, 2), (2, 3), (2, 8), (3, 2), (3, 3), (3, 8)])
def test_kronecker(hip_device, H, K, B):
    for acc in (0, 1, 2):
        g = torch.Generator().manual_seed(H + B + K)
        F = 4
        L = _Layer(hip_device, F, H, B, K, acc, "mirror", 3 if acc == 2 else 0, "normal", g)
        gout = torch.randn(F, B, K ** H, generator=g)
        _call(hip_device, "ck_kronecker_bwd", L.garena.ptr(), torch.from_numpy(L.row_off), gout, F, H, B, K, acc)
        L.check_garena("kronecker", f"H={H} K={K} B={B} acc={acc}", R.kronecker_bwd(L.prior.double(), L.row_off, gout.double(), H, K, acc),
                       R.kronecker_bwd(L.prior, L.row_off, gout, H, K, acc), R.kronecker_grads(gout.double(), H, K))


# -------------------------------------------------------------------------------------------------- ck_categorical_bwd
CAT_SCOPE = np.array([2, 0, 3, 0, 1], dtype=np.int64)  # (non-identity, variable 0 twice)
CAT_GFOLD = np.array([0, 2, 1, 0, 2], dtype=np.int32)  # (five folds on three gradient blocks)
CAT_ORDER = np.array([3, 0, 4, 1, 2], dtype=np.int32)


def _cat_x(B, C, g):
    """(4, B) int32: variable 0 random with marginalised rows (-1) and values >= C; 1 constant; 2 two-valued; 3 random."""
    x = torch.randint(C, (4, B), generator=g, dtype=torch.int32)
    r = torch.rand(B, generator=g)
    x[0, r < 0.15] = -1
    x[0, r > 0.9] = C
    x[0, r > 0.95] = C + 3
    x[1] = C - 1
    x[2] = torch.where(torch.rand(B, generator=g) < 0.5, 0, C - 1).to(torch.int32)
    return x


def _cat_case(dev, kernel, *, B, K, C, acc, gfold, order, seed):
    g = torch.Generator().manual_seed(seed)
    F = 5
    xt = _cat_x(B, C, g)
    gout = torch.randn(3 if gfold else F, B, K, generator=g)
    gout[torch.rand(gout.shape, generator=g) < 0.1] = 0.0
    gf = CAT_GFOLD if gfold else None
    prior = torch.randn(F, C + 1, K, generator=g) if acc else None
    table = _Guarded(F * (C + 1) * K, dev)
    if acc:
        table.out.copy_(prior.reshape(-1))
    _call(dev, "ck_categorical_bwd", gout, None if gf is None else torch.from_numpy(gf), xt, torch.from_numpy(CAT_SCOPE), table.out.data_ptr(), F, B, K, C, acc,
          torch.from_numpy(CAT_ORDER) if order else None)
    got = table.read().view(F, C + 1, K)  # (accumulate = 0: every word of every row, row C included, was written)
    ref = R.categorical_bwd(gout.double(), gf, xt, CAT_SCOPE, C, None if prior is None else prior.double(), acc)
    yard = R.categorical_bwd(gout, gf, xt, CAT_SCOPE, C, prior, acc)
    rows = R.categorical_rows(xt, CAT_SCOPE, C)
    m = torch.zeros(F, C + 1, dtype=torch.float64).scatter_add_(1, rows, torch.ones(F, B, dtype=torch.float64)).unsqueeze(-1)
    mass = R.categorical_bwd(gout.double().abs(), gf, xt, CAT_SCOPE, C, None if prior is None else prior.double().abs(), acc)
    if not acc:
        assert bool((got[(m == 0).expand_as(got)] == 0).all()), "a category nobody selected is not exactly 0"
    _check(kernel, f"K={K} C={C} B={B} acc={acc} gfold={int(gfold)} order={int(order)}", got, ref, yard, m * EPS * mass)


@pytest.mark.parametrize("C", [2, 7, 256])
@pytest.mark.parametrize("K", [1, 3, 4, 12, 33, 32])
def test_categorical_unsorted(hip_device, K, C):
    """K & 3 == 0 (float4 lanes; K = 12: 85 rows a pass and an idle thread) and not; K = 32 stays here below 256 rows."""
    for i, B in enumerate((100,) if K == 32 else (1, 5, 255)):
        for acc in (0, 1):
            _cat_case(hip_device, "categorical:unsorted", B=B, K=K, C=C, acc=acc, gfold=(i + acc) % 2 == 1, order=False, seed=K + C + B)


@pytest.mark.parametrize("C", [2, 256])
@pytest.mark.parametrize("K", [32, 64, 96])
def test_categorical_sorted(hip_device, K, C):
    """B from the threshold of the sorted launch over both sides of its 4096-row chunk to a third, ragged chunk."""
    for i, B in enumerate((256, 257, 4095, 4096, 4097, 8200)):
        for acc in (0, 1):
            _cat_case(hip_device, "categorical:sorted", B=B, K=K, C=C, acc=acc, gfold=(i + acc) % 2 == 1, order=i % 3 != 0, seed=K + C + B)


@pytest.mark.parametrize("B", [100, 300])
def test_categorical_above_48k_of_lds(hip_device, B):
    """C = 256, K = 128: 129 KB of histogram -- unsorted at B = 100, sorted (147 KB) at B = 300."""
    for acc in (0, 1):
        _cat_case(hip_device, "categorical:sorted" if B >= 256 else "categorical:unsorted", B=B, K=128, C=256, acc=acc, gfold=bool(acc), order=B >= 256,
                  seed=B)


def test_categorical_refuses_fold_order_on_the_unsorted_launch(hip_device):
    table = _Guarded(5 * 3 * 4, hip_device)
    with pytest.raises(ValueError, match="fold_order is only read by the sorted launch"):
        _call(hip_device, "ck_categorical_bwd", torch.zeros(5, 8, 4), None, torch.zeros(4, 8, dtype=torch.int32), torch.from_numpy(CAT_SCOPE),
              table.out.data_ptr(), 5, 8, 4, 2, 0, torch.from_numpy(CAT_ORDER))
    assert bool((table.raw() == NAN_BITS).all()), "a refused launch wrote something"


# ----------------------------------------------------------------------------------------------------- ck_gaussian_bwd
@pytest.mark.parametrize("K", [1, 5, 64, 256, 300])
def test_gaussian(hip_device, K):
    """K below, at and above the 256 threads (300: a second pass of 44 units); B below and above the row groups.  Variable 0 is
    NaN in 30 % of the rows, variable 1 in all of them; fold 3 reads variable 0 again; stddev log-uniform over [1e-3, 2]."""
    F, scope = 4, np.array([0, 2, 1, 0], dtype=np.int64)
    groups = 256 // min(K, 256)
    for B in (1, 7, 256, 1000):
        chain = -(-B // groups) + min(groups, B) + 8  # (the roundings an addend can meet: the module docstring)
        g = torch.Generator().manual_seed(K + B)
        xt = torch.randn(3, B, generator=g) * 2
        xt[0, torch.rand(B, generator=g) < 0.3] = float("nan")
        xt[1] = float("nan")
        mean = torch.randn(F, K, generator=g)
        std = torch.exp(torch.rand(F, K, generator=g) * (np.log(2.0) - np.log(1e-3)) + np.log(1e-3))
        gout = torch.randn(F, B, K, generator=g)
        dm, ds = _Guarded(F * K, hip_device), _Guarded(F * K, hip_device)
        _call(hip_device, "ck_gaussian_bwd", gout, xt, torch.from_numpy(scope), mean, std, dm.out.data_ptr(), ds.out.data_ptr(), F, B, K)
        ref = R.gaussian_bwd(gout.double(), xt.double(), scope, mean.double(), std.double())
        yard = R.gaussian_bwd(gout, xt, scope, mean, std)
        masses = [t.sum(1) for t in R.gaussian_terms(gout.double(), xt.double(), scope, mean.double(), std.double(), magnitudes=True)]
        for name, buf, r, y, ms in zip(("dmean", "dstddev"), (dm, ds), ref, yard, masses):
            got = buf.read().view(F, K)
            assert bool((got[2] == 0).all()), "a variable marginalised in every row does not give exactly 0"
            _check("gaussian:" + name, f"K={K} B={B}", got, r, y, chain * EPS * ms)


# ------------------------------------------------------------------------------------------------- ck_segment_add_rows
@pytest.mark.parametrize("block_elems", [5, 8, 4 * 1024 * 256 + 4, 4 * 4096 * 256 + 4, 4096 * 256 + 5])
def test_segment_add_rows(hip_device, block_elems):
    """Children with 0, 1 and 5 entries of `clist`; block_elems % 4 == 0 (float4) and not.  grid.x is ceil(work / 256) capped at
    4096 with work = block_elems / 4 on the float4 path and block_elems on the scalar one (ck_backward.hip:1484-1485), so
    4 * 1024 * 256 + 4 is 1025 blocks of float4s, below the cap, with one float4 in the last; 4 * 4096 * 256 + 4 would be 4097
    blocks and 4096 * 256 + 5 scalars 4097: both are capped, and the first threads take a second turn of the stride loop
    (574-575, 587-588).  The large blocks draw their entries from three rows of `tmp`, some of them twice.  Additions in list
    order: the fp32 run of the restatement, bit for bit."""
    g = torch.Generator().manual_seed(block_elems % 1000)
    n = block_elems
    rows = 6 if n < 1 << 20 else 3
    tmp = torch.randn(rows * n, generator=g)
    cptr, clist = np.array([0, 0, 1, 6], dtype=np.int32), (np.array([3, 0, 5, 1, 2, 4]) % rows).astype(np.int32)
    ga = _GuardedArena([n] * 4, hip_device)  # (block 2 is nobody's)
    prior = ga.fill([torch.randn(n, generator=g) for _ in range(4)])
    coff = np.array([ga.off[1], ga.off[3], ga.off[0]], dtype=np.int64)
    _call(hip_device, "ck_segment_add_rows", tmp, torch.from_numpy(cptr), torch.from_numpy(clist), torch.from_numpy(coff), ga.ptr(), 3, n)
    got = ga.read([1, 3, 0])
    yard = R.segment_add_rows(tmp, cptr, clist, coff, prior, n)
    ref = R.segment_add_rows(tmp.double(), cptr, clist, coff, prior.double(), n)
    own = ga.block_mask([0, 1, 3])
    assert torch.equal(got[own].view(torch.int32), yard[own].view(torch.int32)), "not the additions in list order, one fp32 rounding each"
    assert torch.equal(got[ga.block_mask([1])].view(torch.int32), prior[ga.block_mask([1])].view(torch.int32)), "a child without entries changed"
    _check("segment_add_rows", f"block_elems={n}", got[own].view(3, n), ref[own].view(3, n), yard[own].view(3, n))
