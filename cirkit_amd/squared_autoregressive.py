"""Autoregressive conditionals, log probabilities and coding tables of a squared circuit ``p(x) = |c(x)|^2 / Z``
(`HipSquaredCircuit.autoregressive_conditionals`, `.autoregressive_log_probs`, `.coding_tables`; DESIGN.md section 11,
"Autoregressive conditionals and coding of squared circuits").

Step ``i`` of an order ``o`` of the variables is the all-state marginal of ``o_i`` with ``o_0 .. o_{i-1}`` observed and the later
variables integrated out: a step of the exact sampler (cirkit_amd/squared_sampling.py), whose plans, sibling classes and stacked
level tables (`_Sampler.order_plan`, `bind`) are reused as they are.  The sampler cannot know the row before it has drawn it and
runs ``c``'s forward once per step.  Here the row is known, and in `tree_order` every sibling of a path is entirely before the
step's variable (RANK-1: lifted from ``c``'s arena evaluated on the COMPLETE row -- the same values at every step) or entirely
after it (CONST: the partition-function circuit), so per chunk of rows there is ONE forward of ``c`` and ONE launch over
(row, step) (`ck_squared_path_steps`, cirkit_amd/csrc/ck_sqar.hip).  A step whose siblings are split by the order (another order,
`integrate_vars` scattered through the image) first runs its `ck_squared_mixed_fwd` launches -- they read that same forward -- and
then the same kernel on that one step.  Nothing here waits for the device.

Conventions of the squared stack: one `integrate_vars` set per call, integrated out at every step; `order` a permutation of
the other variables (default: `tree_order` restricted to them).  A row with a negative or out-of-range entry at a variable the
selected steps observe -- ``order[:max(positions)]``, and ``order[max(positions)]`` itself for the log probabilities, which read
it -- is NaN in every entry (a uniform coding table); entries at later variables are ignored, which is how a decoder asks for
step ``i`` with the rest of the row still unknown.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _capi as capi
from .autoregressive import check_positions, check_precision
from .squared import _mask_of
from .squared_sampling import sampler

_WORDS = capi.CK_SQ_STEP_LEAF_WORDS
_SCRATCH_BYTES = 1 << 28  # the (rows, steps, C) block one launch of the conditionals / the tables fills
_MAX_STEPS = 65535  # steps of one launch (blockIdx.y)


def check_query(sq, order, positions, integrate_vars=None, precision=None):
    """(sampler, order plan, order ids, selected steps, integrated mask, widest state count): every refusal, before anything
    is allocated.  ``NotImplementedError``: Gaussian inputs, ancestries that are not paths.  ``ValueError``: an order that is
    no permutation of the variables outside `integrate_vars`, bad positions, a bad precision, nothing to order."""
    sm = sampler(sq)
    D = sq.plan.num_variables
    mask = _mask_of(integrate_vars, D)
    free = np.nonzero(~mask)[0].tolist()
    if not free:
        raise ValueError("every variable is integrated out: no step is left")
    if order is None:
        ids = [int(v) for v in sq.graph.tree_order() if not mask[v]]
    else:
        if isinstance(order, torch.Tensor):
            order = order.reshape(-1).cpu().tolist()
        ids = [int(v) for v in np.asarray(order).reshape(-1).tolist()]
    if sorted(ids) != free:
        raise ValueError("order must be a permutation of the variables that are not integrated out")
    steps = check_positions(len(ids), positions)
    op = sm.order_plan(ids, mask)
    C = max(sq.graph.num_states(v) for v in ids)
    if precision is not None:
        check_precision(precision, C)
    return sm, op, ids, steps, mask, C


def _states(sq) -> torch.Tensor:
    """(D,) int64 on the device: the state count of every variable (0 where no single input fold reads it)."""
    st = getattr(sq, "_ar_states", None)
    if st is None:
        n = np.zeros(sq.plan.num_variables, dtype=np.int64)
        for v in range(len(n)):
            try:
                n[v] = sq.graph.num_states(v)
            except NotImplementedError:
                pass
        st = sq._ar_states = (torch.from_numpy(n).to(sq.device), torch.from_numpy(n.astype(np.int32)).to(sq.device))
    return st


def _leaf_words(sq, op, tb):
    """The per-step leaf words of `ck_squared_path_steps` on the host and on the device, kept with the `PathTables`."""
    tables = {}
    for s in op.steps:
        if s.path.leaf[0] not in tables:
            tables[s.path.leaf[0]] = sq._leaf_table(s.path.leaf[0])
    key = tuple(t[0].data_ptr() for t in tables.values())
    if tb.leaf is None or tb.leaf[0] != key:
        host = np.zeros((len(op.steps), _WORDS), dtype=np.int64)
        for si, s in enumerate(op.steps):
            pl, fl = s.path.leaf
            table, C, K, tlog = tables[pl]
            host[si, :7] = (table.data_ptr(), fl, C, K, tlog, s.path.var, len(s.path.levels))
        tb.leaf = (key, host, torch.from_numpy(host).to(sq.device))
    return tb.leaf[1], tb.leaf[2]


def _groups(steps: list[int], mixed, limit: int) -> list[tuple[int, int, int]]:
    """(output column, first step, number of steps) per launch: runs of consecutive steps without mixed folds, at most `limit`
    long; a step with mixed folds alone."""
    out: list[tuple[int, int, int]] = []
    for j, s in enumerate(steps):
        if out and mixed[s] is None:
            j0, s0, n = out[-1]
            if mixed[s0] is None and s0 + n == s and n < limit:
                out[-1] = (j0, s0, n + 1)
                continue
        out.append((j, s, 1))
    return out


def _run(sq, x, order, positions, integrate_vars, rows_per_chunk, what: str, precision=None, steps_per_chunk=None) -> torch.Tensor:
    sm, op, ids, steps, mask, C = check_query(sq, order, positions, integrate_vars, precision if what == "tables" else None)
    D = sq.plan.num_variables
    if x.dim() != 2 or x.shape[1] != D:
        raise ValueError(f"expected x of shape (B, {D}), found {tuple(x.shape)}")
    if steps_per_chunk is not None and int(steps_per_chunk) <= 0:
        raise ValueError("steps_per_chunk must be positive")
    step_rows = sq._chunk_rows(rows_per_chunk, lambda: sm.row_bytes(op))
    dev = sq.device
    B, P = int(x.shape[0]), len(steps)
    if B == 0:
        raise ValueError("x holds no row")
    # the rows: an entry that is no state reads 0 in c's forward; it spoils the row where a selected step observes the variable
    read = np.zeros(D, dtype=bool)
    read[ids[: steps[-1] + (1 if what == "log_prob" else 0)]] = True
    states64, states32 = _states(sq)
    xd = x.to(dev).to(torch.int64)
    no_state = (xd < 0) | (xd >= states64[None, :])
    bad = (no_state & torch.from_numpy(read).to(dev)[None, :]).any(dim=1).to(torch.int32).contiguous()
    xw = torch.where(no_state, torch.zeros((), dtype=torch.int64, device=dev), xd).contiguous()
    if what == "log_prob":
        result = torch.empty((B, P), dtype=torch.float32, device=dev)
    elif what == "tables":
        result = torch.empty((B, P, C + 1), dtype=torch.int32, device=dev)
    else:
        result = torch.empty((B, P, C), dtype=torch.float32, device=dev)
    rows = min(B, step_rows)
    limit = _MAX_STEPS if what == "log_prob" else max(1, min(_MAX_STEPS, _SCRATCH_BYTES // (rows * (C + 1) * 4)))
    if steps_per_chunk is not None:
        limit = min(limit, int(steps_per_chunk))
    order_vars = torch.tensor(ids, dtype=torch.int32).to(dev) if what == "tables" else None
    scratch = None
    bd_z = sq._z_binding()
    stream = torch.cuda.current_stream(dev).cuda_stream
    sq.last_mixed_launches = 0
    for r0 in range(0, B, step_rows):
        xc = xw[r0: r0 + step_rows]
        Bc = int(xc.shape[0])
        bd_c = sq.c._run(xc)  # ONE forward of c for every step of these rows
        tb = sm.bind(op, Bc, bd_c, bd_z)
        leaf_host, leaf_dev = _leaf_words(sq, op, tb)
        arena = tb.arena
        head = (None if arena is None else arena.data_ptr(), bd_z.arena.data_ptr(), bd_c.arena.data_ptr(), tb.host.ctypes.data,
                tb.dev.data_ptr(), int(tb.host.shape[1] * tb.host.shape[2]), op.max_siblings, leaf_host.ctypes.data, leaf_dev.data_ptr())
        tail = (C, Bc, sq.rows_per_block, 1 if sq._complex else 0, stream)
        for j0, s0, n in _groups(steps, tb.launches, limit):
            if tb.launches[s0] is not None:
                sq.last_mixed_launches += sq._launch_mixed(tb.launches[s0], arena, tb.mid, bd_c, bd_z, Bc)
            outs = [None, 0, 0, None, 0, 0, None, 0, 0]
            if what == "log_prob":
                outs[6:] = (result[r0, j0:].data_ptr(), P, 1)
            elif what == "tables":
                if scratch is None:
                    scratch = torch.empty(rows * min(limit, P) * C, dtype=torch.float32, device=dev)
                p = scratch[: Bc * n * C].view(Bc, n, C)
                outs[3:6] = (p.data_ptr(), n * C, C)
            else:
                at = 0 if what == "log_m" else 3
                outs[at: at + 3] = (result[r0, j0:].data_ptr(), P * C, C)
            with torch.cuda.device(dev):
                capi.call("ck_squared_path_steps", *head, s0, n, xc.data_ptr(), D, bad[r0:].data_ptr(), *outs, *tail)
                if what == "tables":
                    torch.exp_(p)
                    whole = n == P
                    q = result[r0: r0 + Bc] if whole else torch.empty((Bc, n, C + 1), dtype=torch.int32, device=dev)
                    capi.call("ck_ar_quantise", p.data_ptr(), order_vars[s0: s0 + n].repeat(Bc).data_ptr(), states32.data_ptr(), Bc * n, C,
                              int(precision), q.data_ptr(), stream)
                    if not whole:
                        result[r0: r0 + Bc, j0: j0 + n] = q
    return result


def autoregressive_conditionals(sq, x, order=None, *, positions=None, integrate_vars=None, rows_per_chunk=None,
                                steps_per_chunk=None) -> torch.Tensor:
    return _run(sq, x, order, positions, integrate_vars, rows_per_chunk, "cond", steps_per_chunk=steps_per_chunk)


def autoregressive_state_log_marginals(sq, x, order=None, *, positions=None, integrate_vars=None, rows_per_chunk=None,
                                       steps_per_chunk=None) -> torch.Tensor:
    """(B, P, C): the un-normalised ``log m`` of every step -- column ``j`` is, bit for bit, ``state_log_marginals(x, order[i],
    order[i + 1:] + integrate_vars, normalized=False)`` at ``i = positions[j]`` (-inf past a variable's own states)."""
    return _run(sq, x, order, positions, integrate_vars, rows_per_chunk, "log_m", steps_per_chunk=steps_per_chunk)


def autoregressive_log_probs(sq, x, order=None, *, positions=None, integrate_vars=None, rows_per_chunk=None) -> torch.Tensor:
    return _run(sq, x, order, positions, integrate_vars, rows_per_chunk, "log_prob")


def coding_tables(sq, x, order=None, *, positions=None, integrate_vars=None, precision: int = 16, rows_per_chunk=None,
                  steps_per_chunk=None) -> torch.Tensor:
    return _run(sq, x, order, positions, integrate_vars, rows_per_chunk, "tables", precision, steps_per_chunk)
