"""The range ANS coder of cirkit_amd/codec.py on the CPU, driven through its provider interface by the tables of the fp64
restatement (tests/autoregressive_restatement.py): exact round trips, the length bound derived in codec.py, corrupt blobs."""
import numpy as np
import pytest

from autoregressive_restatement import covered, quantise, restated_tables
from cirkit_amd import codec
from test_autoregressive_restatement import evidence
from test_loo_restatement import any_case


def _fixed_tables(cum):
    """A provider that ignores what was decoded so far: step i reads cum[i] (B, C + 1)."""
    return lambda step, xs: cum[step]


def _random_tables(rng, steps, B, C, precision, skew=0.3):
    p = rng.dirichlet(np.full(C, skew), size=(steps, B)).astype(np.float32)
    return [quantise(p[i], np.full(B, C), precision) for i in range(steps)]


@pytest.mark.parametrize("precision,C,steps", [(8, 2, 40), (10, 256, 30), (16, 17, 200), (16, 256, 784), (24, 256, 100)])
def test_round_trip_and_length_bound_on_fixed_tables(precision, C, steps):
    rng = np.random.default_rng(51)
    B = 7
    cum = _random_tables(rng, steps, B, C, precision)
    x = np.stack([[rng.choice(C, p=np.diff(cum[i][b]) / (1 << precision)) for i in range(steps)] for b in range(B)])
    x[0] = [int(np.diff(cum[i][0]).argmin()) for i in range(steps)]  # the least likely symbol every time: the longest blob
    order = list(range(steps))
    blobs, counts = codec.encode(_fixed_tables(cum), x, order, precision=precision, return_counts=True)
    assert len(blobs) == B and all(isinstance(b, bytes) for b in blobs)
    back = codec.decode(_fixed_tables(cum), blobs, order, steps, precision=precision)
    assert back.dtype == np.int64 and np.array_equal(back, x)
    ideal = codec.ideal_bits(counts, precision)
    want = np.array([[np.diff(cum[i][b])[x[b, i]] for i in range(steps)] for b in range(B)])
    assert np.array_equal(counts, want)
    bits = np.array([8 * len(b) for b in blobs])
    print(f"  precision {precision}, C {C}, {steps} steps: blob bits - ideal in [{(bits - ideal).min():.2f}, {(bits - ideal).max():.2f}]")
    assert steps <= codec.max_steps(precision)
    assert (bits <= ideal + codec.OVERHEAD_BITS).all()
    # (the other side of the same potential argument: the final state is below 2^63, so the 64 + 32 w bits written hold the
    #  tables' own code length as long as the per-step rounding stays under one unit, which `max_steps` guarantees)
    assert (bits >= ideal).all()


def test_overhead_is_the_state_plus_one_renormalisation_unit():
    assert codec.OVERHEAD_BITS == codec.STATE_BITS + codec.UNIT_BITS == 96 and codec.LOW == 1 << 31
    for n in (8, 16, 24):
        eps = np.log2(1 + 2.0 ** (n - 31))
        assert codec.max_steps(n) * eps <= codec.UNIT_BITS < (codec.max_steps(n) + 1) * eps
    with pytest.raises(ValueError, match="symbols per row"):
        codec.encode(lambda i, xs: None, np.zeros((1, 3000), dtype=np.int64), list(range(3000)), precision=24)


@pytest.mark.parametrize("name", ["kat_bernoulli_f0o0", "kat_bernoulli_f1o1", "quadtree_4x4_kron_k3", "binomial_qg6x6_k4"])
def test_round_trip_through_the_restatement(name):
    plan, tensors = any_case(name)
    D = plan.num_variables
    x = evidence(plan, 3, 52).astype(np.int64)
    for order in (covered(plan), [int(v) for v in np.random.default_rng(53).permutation(covered(plan))]):
        tables = restated_tables(plan, tensors, order, 16)
        blobs, counts = codec.encode(tables, x, order, precision=16, return_counts=True)
        back = codec.decode(tables, blobs, order, D, precision=16)
        assert np.array_equal(back, x)
        bits = np.array([8 * len(b) for b in blobs])
        assert (bits <= codec.ideal_bits(counts, 16) + codec.OVERHEAD_BITS).all()


def test_a_flipped_bit_raises_or_decodes_to_something_else():
    rng = np.random.default_rng(54)
    steps, B, C, precision = 60, 2, 17, 12
    cum = _random_tables(rng, steps, B, C, precision, skew=1.0)
    x = rng.integers(0, C, size=(B, steps))
    order = list(range(steps))
    blobs = codec.encode(_fixed_tables(cum), x, order, precision=precision)
    raised = wrong = 0
    for bit in range(0, 8 * len(blobs[0]), 3):
        bad = bytearray(blobs[0])
        bad[bit // 8] ^= 1 << (bit % 8)
        try:
            got = codec.decode(_fixed_tables(cum), [bytes(bad), blobs[1]], order, steps, precision=precision)
        except ValueError:
            raised += 1
            continue
        wrong += 1
        assert not np.array_equal(got[0], x[0]) and np.array_equal(got[1], x[1])
        assert got.min() >= 0 and got.max() < C
    assert raised + wrong > 0 and raised > 0
    for bad in ([b"", blobs[1]], [blobs[0][:-1], blobs[1]], [blobs[0][:-4], blobs[1]], [blobs[0] + b"\0\0\0\0", blobs[1]],
                [b"\0" * 8 + blobs[0][8:], blobs[1]], []):
        with pytest.raises(ValueError):
            codec.decode(_fixed_tables(cum), bad, order, steps, precision=precision)


def test_the_coder_refuses_what_it_cannot_code():
    cum = [quantise(np.array([[0.5, 0.5, 0.0]], dtype=np.float32), np.array([2]), 8)]
    enc = lambda x, **kw: codec.encode(_fixed_tables(cum), np.asarray(x), [0], **{"precision": 8, **kw})  # noqa: E731
    assert codec.decode(_fixed_tables(cum), enc([[1]]), [0], 1, precision=8).tolist() == [[1]]
    for x in ([[2]], [[3]], [[-1]]):  # no count, outside the table, missing
        with pytest.raises(ValueError):
            enc(x)
    with pytest.raises(ValueError):
        enc([[0.5]])
    for p in (7, 25):
        with pytest.raises(ValueError):
            enc([[1]], precision=p)
    broken = [cum[0].copy()]
    broken[0][0, 1] = 300  # not non-decreasing up to the total
    with pytest.raises(ValueError, match="cumulative"):
        codec.encode(_fixed_tables(broken), np.array([[1]]), [0], precision=8)
    with pytest.raises(ValueError, match="shape"):
        codec.encode(lambda i, xs: np.zeros((2, 3)), np.array([[1]]), [0], precision=8)
