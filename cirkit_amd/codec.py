"""Lossless compression with a circuit: `compress` / `decompress` ("Autoregressive conditionals and
coding").

The model side is `HipCircuit.coding_tables`, or `HipSquaredCircuit.coding_tables` for a squared circuit ``|c(x)|^2 / Z`` (order
``None`` is then its `tree_order`; `compress` / `decompress` take either class): per row and step of an order of the variables, the integer cumulative
frequency table of ``p(X_{order[i]} | x_{order[:i]})``.  The coder side is here: a range ANS coder (Duda's rANS in its
64-bit-state, 32-bit-renormalisation form) in numpy, one stream per row, vectorised over the rows, with no GPU dependency --
it takes its tables through a provider callable ``tables(step, x_so_far) -> (B, C + 1)``, so the CPU tests drive it from the
fp64 restatement and `compress` / `decompress` from the GPU.

Parameters of the coder: the state is a uint64 kept in ``[L, L 2**32)`` with ``L = 2**31`` between symbols; encoding symbol
``s`` of frequency ``f`` and start ``c`` at precision ``n`` (``T = 2**n``) first emits the low 32 bits of the state while it is
``>= f 2**(63 - n)`` (at most once, because ``n <= 24 < 32``) and then maps ``x -> (x // f) T + x % f + c``.  Symbols are
encoded last to first, so that the decoder reads them first to last.  A blob is the final state (8 bytes, little endian)
followed by the emitted words in decoding order (4 bytes each, little endian).

Length of a blob.  With ``Phi = log2(state) + 32 (words emitted)``: a renormalisation does not raise ``Phi``, and an encoding
step raises it by less than ``log2(T / f) + eps`` with ``eps = log2(1 + 2**(n - 31))`` (the state is at least ``f L / T``
before the step).  ``Phi`` starts at 31 and the final state is at least ``L``, so the words carry fewer than ``sum_i log2(T /
f_i) + steps eps`` bits and the blob, with its 64 bits of state, fewer than ``ideal + 64 + steps eps``.  `OVERHEAD_BITS` = 96 is
the state width plus one renormalisation unit: the bound ``8 len(blob) <= ideal + OVERHEAD_BITS`` holds for every row of at
most `max_steps(precision)` symbols (``steps eps <= 32``: 2850 symbols at precision 24, 726 828 at 16), and longer rows are
refused.
"""

from __future__ import annotations

from typing import TYPE_CHECKING, Callable

import numpy as np

if TYPE_CHECKING:  # pragma: no cover
    from .circuit import HipCircuit

STATE_BITS = 64  # the final state, written out whole
UNIT_BITS = 32  # one renormalisation unit
LOW = 1 << 31  # L: the lower bound of the state between symbols
OVERHEAD_BITS = STATE_BITS + UNIT_BITS  # 8 len(blob) <= sum_i -log2(f_i / T) + OVERHEAD_BITS

_U = np.uint64
_MASK32 = _U(0xFFFFFFFF)

Tables = Callable[[int, np.ndarray], np.ndarray]


def max_steps(precision: int) -> int:
    """The longest row for which `OVERHEAD_BITS` bounds the blob: ``steps log2(1 + 2**(precision - 31)) <= 32``."""
    return int(UNIT_BITS / np.log2(1.0 + 2.0 ** (int(precision) - 31)))


def _check_precision(precision: int) -> int:
    if isinstance(precision, bool) or int(precision) != precision or not 8 <= int(precision) <= 24:
        raise ValueError(f"precision {precision!r} outside 8 .. 24")
    return int(precision)


def _table(tables: Tables, step: int, xs: np.ndarray, B: int, T: int) -> np.ndarray:
    """The provider's (B, C + 1) table of a step as int64, checked: 0 first, T last, non-decreasing."""
    t = tables(step, xs)
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    t = np.asarray(t).astype(np.int64)
    if t.ndim != 2 or t.shape[0] != B or t.shape[1] < 2:
        raise ValueError(f"step {step}: the table provider returned shape {t.shape}, expected ({B}, C + 1)")
    if (t[:, 0] != 0).any() or (t[:, -1] != T).any() or (np.diff(t, axis=1) < 0).any():
        raise ValueError(f"step {step}: not a cumulative frequency table of total {T}")
    return t


def encode(tables: Tables, x, order, *, precision: int = 16, return_counts: bool = False):
    """One byte string per row of `x` (B, D) integers: the symbols ``x[:, order[i]]`` under the tables ``tables(i, x_so_far)``,
    where ``x_so_far`` is `x` with every variable at a step ``>= i`` (and every variable outside the order) set to -1 -- what
    the decoder holds at that step.  ``ValueError``: a symbol outside its table or with no count, a row longer than
    `max_steps`.  With `return_counts` also the (B, steps) counts ``f_i`` of the coded symbols."""
    n = _check_precision(precision)
    T = 1 << n
    x = np.asarray(x)
    if x.ndim != 2 or x.dtype.kind not in "iu":
        raise ValueError("x must be a (B, D) integer array")
    x = x.astype(np.int64)
    order = [int(v) for v in order]
    B, steps = x.shape[0], len(order)
    if steps > max_steps(n):
        raise ValueError(f"{steps} symbols per row exceed the {max_steps(n)} that precision {n} bounds; lower the precision")
    start, freq = np.empty((B, steps), dtype=np.int64), np.empty((B, steps), dtype=np.int64)
    xs = np.full_like(x, -1)
    rows = np.arange(B)
    for i, v in enumerate(order):
        t = _table(tables, i, xs, B, T)
        s = x[:, v]
        if (s < 0).any() or (s >= t.shape[1] - 1).any():
            raise ValueError(f"step {i}: variable {v} holds a symbol outside 0 .. {t.shape[1] - 2} (missing values cannot be coded)")
        start[:, i], freq[:, i] = t[rows, s], t[rows, s + 1] - t[rows, s]
        if (freq[:, i] <= 0).any():
            raise ValueError(f"step {i}: variable {v} holds a symbol its table gives no count")
        xs[:, v] = s
    state = np.full(B, LOW, dtype=_U)
    words = np.zeros((B, max(1, steps)), dtype=np.uint32)
    count = np.zeros(B, dtype=np.int64)
    for i in range(steps - 1, -1, -1):
        f, c = freq[:, i].astype(_U), start[:, i].astype(_U)
        full = state >= (f << _U(63 - n))
        if full.any():
            words[full, count[full]] = (state[full] & _MASK32).astype(np.uint32)
            count[full] += 1
            state[full] >>= _U(32)
        state = ((state // f) << _U(n)) + (state % f) + c
    blobs = [state[b].astype("<u8").tobytes() + words[b, : count[b]][::-1].astype("<u4").tobytes() for b in range(B)]
    return (blobs, freq) if return_counts else blobs


def decode(tables: Tables, blobs, order, num_variables: int, *, precision: int = 16) -> np.ndarray:
    """(B, num_variables) int64: the rows `encode` coded (variables outside the order read 0).  ``ValueError`` for blobs that
    do not decode: a malformed length, a state out of range, a stream that runs out or is not used up, a final state that is
    not the coder's initial one.  A corrupt blob raises or returns wrong symbols; every index is taken inside its table."""
    n = _check_precision(precision)
    T = 1 << n
    order = [int(v) for v in order]
    B, D = len(blobs), int(num_variables)
    if B == 0:
        raise ValueError("no blobs")
    if any(not isinstance(b, (bytes, bytearray)) or len(b) < 8 or (len(b) - 8) % 4 for b in blobs):
        raise ValueError("blobs do not decode: each is 8 bytes of state and a whole number of 4-byte words")
    state = np.array([np.frombuffer(bytes(b[:8]), dtype="<u8")[0] for b in blobs], dtype=_U)
    if (state < _U(LOW)).any() or (state >= _U(1 << 63)).any():
        raise ValueError("blobs do not decode: a state outside the coder's range")
    length = np.array([(len(b) - 8) // 4 for b in blobs], dtype=np.int64)
    words = np.zeros((B, max(1, int(length.max()))), dtype=_U)
    for b, blob in enumerate(blobs):
        words[b, : length[b]] = np.frombuffer(bytes(blob[8:]), dtype="<u4")
    at = np.zeros(B, dtype=np.int64)
    rows = np.arange(B)
    xs = np.full((B, D), -1, dtype=np.int64)
    for i, v in enumerate(order):
        t = _table(tables, i, xs, B, T)
        slot = (state & _U(T - 1)).astype(np.int64)
        s = (t[:, 1:] <= slot[:, None]).sum(axis=1)  # (t[:, -1] = T > slot: s <= C - 1, and t[s] <= slot < t[s + 1])
        c, f = t[rows, s], t[rows, s + 1] - t[rows, s]
        state = f.astype(_U) * (state >> _U(n)) + (slot - c).astype(_U)
        low = state < _U(LOW)
        if low.any():
            if (at[low] >= length[low]).any():
                raise ValueError("blobs do not decode: a stream ends before its row does")
            state[low] = (state[low] << _U(32)) | words[low, at[low]]
            at[low] += 1
        xs[:, v] = s
    if (at != length).any() or (state != _U(LOW)).any():
        raise ValueError("blobs do not decode: a stream is not used up by its row")
    xs[xs < 0] = 0
    return xs


def ideal_bits(counts: np.ndarray, precision: int) -> np.ndarray:
    """(B,) ``sum_i -log2(f_i / 2**precision)``: what the quantised tables ask for the coded symbols."""
    return (int(precision) - np.log2(np.asarray(counts, dtype=np.float64))).sum(axis=1)


# -- the circuit as the provider ----------------------------------------------------------------------------------------------
def _squared(hc) -> bool:
    from .squared import HipSquaredCircuit

    return isinstance(hc, HipSquaredCircuit)


def _order(hc: "HipCircuit", order) -> list[int]:
    from .autoregressive import check_order
    from .topdown import variable_kinds

    if _squared(hc):  # (a permutation of all variables; None: `tree_order`)
        from .squared_autoregressive import check_query

        return check_query(hc, order, None)[2]
    return check_order(variable_kinds(hc.plan), hc.plan.num_variables, order)


def _check(hc: "HipCircuit", order, precision: int) -> list[int]:
    from .autoregressive import check_precision, state_counts
    from .sampling import check_plan
    from .topdown import variable_kinds

    if _squared(hc):  # (Gaussian inputs and ancestries that are no paths are refused by `check_query`; every input is discrete)
        from .squared_autoregressive import check_query

        ids = check_query(hc, order, None, None, precision)[2]
        if len(ids) > max_steps(precision):
            raise ValueError(f"{len(ids)} symbols per row exceed the {max_steps(precision)} that precision {precision} bounds")
        return ids
    check_plan(hc.user_plan)
    ids = _order(hc, order)
    if any("gaussian" in variable_kinds(hc.plan)[v] for v in ids):
        raise ValueError("coding takes discrete variables only")
    check_precision(precision, int(state_counts(hc.plan)[ids].max()))
    if len(ids) > max_steps(precision):
        raise ValueError(f"{len(ids)} symbols per row exceed the {max_steps(precision)} that precision {precision} bounds")
    return ids


def stepwise_tables(hc: "HipCircuit", order: list[int], precision: int) -> Tables:
    """The provider both sides use by default: step i is one `coding_tables` call on the B rows held so far."""
    import torch

    def tables(step: int, xs: np.ndarray) -> np.ndarray:
        t = hc.coding_tables(torch.from_numpy(xs).to(hc.device), order, positions=[step], precision=precision)
        return t[:, 0].cpu().numpy()

    return tables


def compress(hc: "HipCircuit", x, order=None, *, precision: int = 16, batched: bool = False, return_counts: bool = False):
    """One byte string per row of ``x`` (B, D) integers (a tensor or an array), coded along `order` (None: the covered
    variables ascending) with the tables of `HipCircuit.coding_tables` at `precision`.  By default the tables come from the
    stepwise calls `decompress` makes, on the same B rows, so that the decoder reproduces the encoder's integers by
    construction; ``batched=True`` takes them from ONE all-steps call instead (bit-identical on the GPU, which
    tests/test_autoregressive.py pins).  Refused before anything is launched: what `coding_tables` refuses, missing values."""
    import torch

    ids = _check(hc, order, precision)
    xn = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if xn.ndim != 2 or xn.dtype.kind not in "iu" or xn.shape[1] < hc.plan.num_variables:
        raise ValueError(f"x must be (B, D) integers over the circuit's {hc.plan.num_variables} variables")
    xn = xn[:, : hc.plan.num_variables].astype(np.int64)
    if (xn[:, ids] < 0).any():
        raise ValueError("missing values cannot be coded")
    if batched:
        full = hc.coding_tables(torch.from_numpy(xn).to(hc.device), ids, precision=precision).cpu().numpy()
        tables = lambda step, xs: full[:, step]  # noqa: E731
    else:
        tables = stepwise_tables(hc, ids, precision)
    return encode(tables, xn, ids, precision=precision, return_counts=return_counts)


def decompress(hc: "HipCircuit", blobs, order=None, *, precision: int = 16):
    """``(B, D)`` int64 tensor on the host: the rows `compress` coded, decoded step by step -- step i asks `coding_tables`
    for the table of ``order[i]`` given the symbols decoded so far, looks the symbol up against the coder state and writes it
    in.  ``ValueError`` for blobs that do not decode."""
    import torch

    ids = _check(hc, order, precision)
    return torch.from_numpy(decode(stepwise_tables(hc, ids, precision), list(blobs), ids, hc.plan.num_variables,
                                   precision=precision))
