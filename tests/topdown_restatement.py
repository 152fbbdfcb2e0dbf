"""The top-down message pass restated in plain torch, one function per entry point of `ck_flow_*`, `ck_loo_*` and `ck_stats_*`
(include/cirkit_hip.h; the formulas are those of the headers of ck_down.h, ck_flow.hip, ck_loo.hip, ck_loo_leaf.h and
ck_stats.hip, not their loops).  Every function takes the raw tables the entry point takes -- `child`, `w`, `val_off`,
`fold_off`, the CSR lists `cstart / cfold / cfirst / items`, the leaf-entry tables of 4 or 5 int64 per entry -- as host tensors
and numpy arrays, and returns what the entry point writes.  Arenas are flat tensors; global fold g's (B, K) block starts at
val_off[g].

`dtype` is the run mode:
* torch.float64: the reference.
* torch.float32: the yardstick, the header formulas as they stand: lg_k = log f_k - v_k is ROUNDED, the factor of a unit is
  exp(lg_k - m), an entry receives T_i exp(m + e_i).
* EXACT32 ("exact-shift fp32"): fp32 arithmetic, except that every exponent the kernels promise not to round -- -v - m, m + e,
  e - v -- is formed in fp64 from the fp32 operands and rounded once before the fp32 exp: the factor is f_k exp(-v_k - m).
  The yardstick of the far-tail family, where log f - v is rounded at the size of v (2^-15 near -700) in the plain run.
* TWOSUM32: EXACT32 without its one rounding: the exponent is split into its fp32 value hi and the remainder lo, and
  x exp(hi + lo) is taken as x exp(hi) (1 + lo) in fp32 -- what ck_down.h promises of `scaled_exp` ("to ~2e-7 relative, whatever
  the size of a and b").  The rounding of an exponent s costs |s| 2^-25 relative, 2e-6 on an entry e^-60 below its row's largest.

The fp32 runs add the Ko products of a contraction T_i = sum_k a_k w[k, i] in unit order, one rounding each, as a plain loop
does (torch's blocked matrix product is up to 20 x closer to fp64 on a sum of 768 terms than any such loop).

tests/test_topdown_restatement.py pins these functions to torch autograd and to the quotient / moment formulas."""
import numpy as np
import torch

SUM, CPT, TUCKER, HADAMARD, KRONECKER = range(2, 7)  # (CK_SAMPLE_* of include/cirkit_hip.h; 0 and 1 are the input layers)
EXACT32 = "exact32"
TWOSUM32 = "twosum32"
NEG_INF = float("-inf")
SMALL = 2.0 ** -120  # a shifted factor below this is what an fp32 factor cannot hold (2^-126 with a margin for the fast log)
SLOW_SHIFT = 40.0    # ck_stats.hip: a row with an entry of e_i + m >= 40 leaves the factored product


def torch_dtype(dtype):
    return torch.float32 if dtype in (EXACT32, TWOSUM32) else dtype


def _c(x, dtype):
    return x.to(torch_dtype(dtype))


def block(arena, val_off, g, B, K):
    o = int(val_off[g])
    return arena[o:o + B * K].view(B, K)


def _zero_where(mask, x):
    return torch.where(mask, x, torch.zeros_like(x))


def mul_exp(x, a, b, dtype):
    """x exp(a + b) for finite a, b with x exp(a + b) representable: the exponent a + b is formed in fp64 and rounded once in
    the EXACT32 run, and its remainder kept as a factor 1 + lo in the TWOSUM32 run; where it reaches 80 (exp alone overflows in
    fp32) the exponential is taken in two halves."""
    if dtype in (EXACT32, TWOSUM32):
        s64 = a.double() + b.double()
        s = s64.float()
    else:
        s = a + b
    big = s >= 80
    h = torch.where(big, s * 0.5, s)
    r = x * torch.exp(h)
    r = torch.where(big, r * torch.exp(h), r)
    if dtype == TWOSUM32:
        r = r + r * (s64 - s.double()).float()
    return r


def lse(x, dim):
    """log-sum-exp over `dim` with one maximum, -inf where every term is."""
    mx = x.amax(dim, keepdim=True)
    fin = torch.isfinite(mx)
    mxs = _zero_where(fin, mx)
    out = mxs + torch.log(torch.exp(x - mxs).sum(dim, keepdim=True).clamp_min(torch.finfo(x.dtype).tiny))
    return torch.where(fin, out, torch.full_like(out, NEG_INF)).squeeze(dim)


def entry_values(type, ch, H, Ki, vals, val_off, B):
    """(B, M) child values of the entries of one fold (ck_walk.h): sum / mixing unit i % Ki of input i / Ki; CP-T unit i of
    every input, added in input order; Tucker v0[i / Ki] + v1[i % Ki]."""
    blk = [block(vals, val_off, int(g), B, Ki) for g in ch[:H]]
    if type == SUM:
        return torch.cat(blk, dim=1)
    if type == CPT:
        e = blk[0]
        for b in blk[1:]:
            e = e + b
        return e
    return (blk[0].unsqueeze(2) + blk[1].unsqueeze(1)).reshape(B, Ki * Ki)


# ------------------------------------------------------------------------------------------------------- the flow pass
def flow_factors(f, v, dtype):
    """a (B, Ko), m (B, 1), ok: lg_k = log f_k - v_k over the units with f_k > 0 and finite v_k, m = max_k lg_k, a_k =
    exp(lg_k - m) = f_k exp(-v_k - m); 0 for a dropped unit; m = -inf when every unit dropped."""
    ok = (f > 0) & torch.isfinite(v)
    one = torch.ones_like(f)
    vs = _zero_where(ok, v)
    lg = torch.where(ok, torch.log(torch.where(ok, f, one)) - vs, torch.full_like(f, NEG_INF))
    m = lg.amax(-1, keepdim=True)
    live = torch.isfinite(m)
    ms = _zero_where(live, m)
    if dtype == torch.float32:  # (the header formula as it stands)
        a = torch.exp(torch.where(ok, lg, torch.zeros_like(lg)) - ms)
    else:
        a = mul_exp(f, -vs, -ms.expand_as(vs), dtype)
    return _zero_where(ok & live, a), m, ok


def _contract(a, wf, diag, H, Ki):
    """T (B, M) = sum_k a_k w[k, i], in fp32 added in unit order; mixing: entry i only meets unit i % Ki."""
    if diag:
        i = torch.arange(wf.shape[1])
        return a.repeat(1, H) * wf[i % Ki, i]
    if a.dtype == torch.float64:
        return a @ wf
    T = torch.zeros(a.shape[0], wf.shape[1])
    for k in range(wf.shape[0]):
        T = T + a[:, k:k + 1] * wf[k]
    return T


def _flow_entries(type, diag, ch, wf, H, Ki, Ko, vals, flow, val_off, g, B, dtype, small):
    """(B, M): what entry i of global fold g receives, T_i exp(m + e_i), exactly 0 where T_i = 0 or e_i = -inf.  `small`: only the
    terms of the units whose shifted factor is below SMALL (the allowance of an fp32 factor; fp64 run)."""
    a, m, _ = flow_factors(block(flow, val_off, g, B, Ko), block(vals, val_off, g, B, Ko), dtype)
    if small:
        a = _zero_where(a < SMALL, a)
    T = _contract(a, wf, diag, H, Ki)
    e = entry_values(type, ch, H, Ki, vals, val_off, B)
    pos = (T > 0) & (e > NEG_INF)
    ms = _zero_where(torch.isfinite(m), m).expand_as(e)
    return _zero_where(pos, mul_exp(T, ms, _zero_where(pos, e), dtype))


def n_slots(type, F, H, flow_pass):
    return F * H if type == SUM or (type == CPT and not flow_pass) else (F if type == CPT else 2 * F)


def flow_down_sum(type, diag, child, w, F, H, Ki, Ko, M, vals, flow, val_off, fold_off, B, dtype, small=False):
    """`ck_flow_down_sum`: msg (slots, B, Ki).  Sum / mixing: slot f H + i / Ki, unit i % Ki; CP-T: slot f, unit i; Tucker: slot
    2 f unit a the sum over b, slot 2 f + 1 unit b the sum over a."""
    vals, flow, w = _c(vals, dtype), _c(flow, dtype), _c(w, dtype).view(F, Ko, M)
    msg = torch.zeros(n_slots(type, F, H, True), B, Ki, dtype=torch_dtype(dtype))
    for f in range(F):
        fl = _flow_entries(type, diag, child[f * H:(f + 1) * H], w[f], H, Ki, Ko, vals, flow, val_off, fold_off + f, B, dtype, small)
        if type == SUM:
            for h in range(H):
                msg[f * H + h] = fl[:, h * Ki:(h + 1) * Ki]
        elif type == CPT:
            msg[f] = fl
        else:
            fl = fl.view(B, Ki, Ki)
            msg[2 * f], msg[2 * f + 1] = fl.sum(2), fl.sum(1)
    return msg


def flow_segment_add(msg, cstart, cfold, cfirst, items, flow, val_off, n_child, Ki, B, dtype):
    """`ck_flow_segment_add`: the flow arena with the (B, Ki) block of every child c = the slots items[cstart[c] ..
    cstart[c + 1] - 1] of msg added in list order, stored where cfirst[c] != 0, added onto the block where it is 0."""
    out, msg = _c(flow, dtype).clone(), _c(msg, dtype)
    for c in range(n_child):
        dst = block(out, val_off, int(cfold[c]), B, Ki)
        acc = torch.zeros_like(dst) if cfirst[c] else dst.clone()
        for s in range(int(cstart[c]), int(cstart[c + 1])):
            acc = acc + msg.view(-1, B, Ki)[int(items[s])]
        dst.copy_(acc)
    return out


def _kron_view(p, B, H, Ki):
    return p.reshape([B] + [Ki] * H)


def flow_down_product(type, cstart, cfold, cfirst, items, flow, val_off, n_child, H, Ki, Ko, B, dtype):
    """`ck_flow_down_product`.  Hadamard: items are the consumers' global folds, unit k receives f_k of each.  Kronecker: items
    are pairs (consumer global fold, input position h), unit i receives the sum of f over the outputs whose digit h (base Ki,
    input 0 most significant) is i."""
    src = _c(flow, dtype)
    out = src.clone()
    for c in range(n_child):
        dst = block(out, val_off, int(cfold[c]), B, Ki)
        acc = torch.zeros_like(dst) if cfirst[c] else dst.clone()
        for s in range(int(cstart[c]), int(cstart[c + 1])):
            if type == HADAMARD:
                acc = acc + block(src, val_off, int(items[s]), B, Ko)
            else:
                g, h = int(items[2 * s]), int(items[2 * s + 1])
                p = _kron_view(block(src, val_off, g, B, Ko), B, H, Ki)
                acc = acc + p.sum([d + 1 for d in range(H) if d != h])
        dst.copy_(acc)
    return out


def row_ok(vals, val_off, root_fold, root_ko, bad, B):
    r = block(vals, val_off, root_fold, B, root_ko)[:, 0]
    return torch.isfinite(r) & (torch.as_tensor(bad) == 0), r


def flow_leaf_categorical(entries, qstart, Q, Cout, ntab, flow, vals, val_off, root_fold, root_ko, bad, B, dtype):
    """`ck_flow_leaf_categorical`: out (B, Q, Cout), logev (B).  out[n, q, c] = sum over the entries of q and their units k of
    f_k ntab[k, c], states c >= C of an entry read 0; NaN rows without a finite root value or with bad[n] != 0; logev the root
    value, NaN where bad."""
    flow, ntab = _c(flow, dtype), _c(ntab, dtype)
    ok, root = row_ok(_c(vals, dtype), val_off, root_fold, root_ko, bad, B)
    out = torch.zeros(B, Q, Cout, dtype=torch_dtype(dtype))
    for q in range(Q):
        for s in range(int(qstart[q]), int(qstart[q + 1])):
            g, K, C, off = (int(x) for x in entries[s][:4])
            c = min(C, Cout)
            out[:, q, :c] += block(flow, val_off, g, B, K) @ ntab[off:off + K * C].view(K, C)[:, :c]
    out[~ok] = float("nan")
    return out, torch.where(torch.as_tensor(bad) != 0, torch.full_like(root, float("nan")), root)


def flow_leaf_gaussian(entries, qstart, Q, mean, stddev, flow, vals, val_off, root_fold, root_ko, bad, B, dtype):
    """`ck_flow_leaf_gaussian`: out (B, Q, 2) = (S1, S2 - S1^2), S1 = sum f_k mean_k, S2 = sum f_k (stddev_k^2 + mean_k^2)."""
    flow, mean, stddev = _c(flow, dtype), _c(mean, dtype), _c(stddev, dtype)
    ok, root = row_ok(_c(vals, dtype), val_off, root_fold, root_ko, bad, B)
    s1 = torch.zeros(B, Q, dtype=torch_dtype(dtype))
    s2 = torch.zeros_like(s1)
    for q in range(Q):
        for s in range(int(qstart[q]), int(qstart[q + 1])):
            g, K, _, off = (int(x) for x in entries[s][:4])
            fr, mu, sd = block(flow, val_off, g, B, K), mean[off:off + K], stddev[off:off + K]
            s1[:, q] += fr @ mu
            s2[:, q] += fr @ (sd * sd + mu * mu)
    out = torch.stack([s1, s2 - s1 * s1], -1)
    out[~ok] = float("nan")
    return out, torch.where(torch.as_tensor(bad) != 0, torch.full_like(root, float("nan")), root)


def observed(ev, x_float, gaussian=False):
    """Sentinels: a negative int64; in fp32 NaN, or for a discrete variable a value <= -1 (a float batch is truncated)."""
    if not x_float:
        return ev >= 0
    return ~torch.isnan(ev) if gaussian else ev > -1.0


def flow_check_evidence(ev, x_float, states, B, D):
    """`ck_flow_check_evidence`: clean (B, D), bad (B) int32, flag: an observed category at or beyond states[d] > 0 is out of
    range; it is replaced by 0, its row marked."""
    S = torch.as_tensor(states).view(1, D)
    oor = (S > 0) & observed(ev, x_float) & (ev >= S.to(ev.dtype))
    clean = torch.where(oor, torch.zeros_like(ev), ev)
    bad = oor.any(1).to(torch.int32)
    return clean, bad, int(bad.any())


# ------------------------------------------------------------------------------------------------- the derivative pass
def loo_down_sum(type, diag, child, w, F, H, Ki, Ko, M, vals, der, val_off, fold_off, B, dtype):
    """`ck_loo_down_sum`: msg (slots, B, Ki).  m = max_k D_k over the finite D_k, T_i = sum_k w[k, i] exp(D_k - m), base_i =
    m + log T_i (-inf where T_i = 0).  Sum / mixing: slot f H + i / Ki unit i % Ki holds base_i; CP-T: slot f H + h unit i holds
    base_i plus the values of the inputs h' != h at unit i, added in input order; Tucker: slot 2 f unit a holds
    lse_b(base_(a, b) + v_1[b]), slot 2 f + 1 unit b holds lse_a(base_(a, b) + v_0[a])."""
    vals, der, w = _c(vals, dtype), _c(der, dtype), _c(w, dtype).view(F, Ko, M)
    msg = torch.zeros(n_slots(type, F, H, False), B, Ki, dtype=torch_dtype(dtype))
    ninf = torch.tensor(NEG_INF, dtype=torch_dtype(dtype))
    for f in range(F):
        ch = child[f * H:(f + 1) * H]
        d = block(der, val_off, fold_off + f, B, Ko)
        fin = torch.isfinite(d)
        m = torch.where(fin, d, ninf).amax(-1, keepdim=True)
        live = torch.isfinite(m)
        ms = _zero_where(live, m)
        a = _zero_where(fin, torch.exp(_zero_where(fin, d) - ms))
        T = _contract(a, w[f], diag, H, Ki)
        base = torch.where(T > 0, ms + torch.log(torch.where(T > 0, T, torch.ones_like(T))), ninf)
        if type == SUM:
            for h in range(H):
                msg[f * H + h] = base[:, h * Ki:(h + 1) * Ki]
        elif type == CPT:
            for h in range(H):
                acc = base
                for h2 in range(H):
                    if h2 != h:
                        acc = acc + block(vals, val_off, int(ch[h2]), B, Ki)
                msg[f * H + h] = acc
        else:
            base = base.view(B, Ki, Ki)
            v0, v1 = block(vals, val_off, int(ch[0]), B, Ki), block(vals, val_off, int(ch[1]), B, Ki)
            msg[2 * f] = lse(base + v1.unsqueeze(1), 2)
            msg[2 * f + 1] = lse(base + v0.unsqueeze(2), 1)
    return msg


def loo_segment_lse(msg, cstart, cfold, cfirst, items, der, val_off, n_child, Ki, B, dtype):
    """`ck_loo_segment_lse`: logaddexp over the child's slots in list order, stored (cfirst) or combined with the block."""
    out, msg = _c(der, dtype).clone(), _c(msg, dtype)
    for c in range(n_child):
        dst = block(out, val_off, int(cfold[c]), B, Ki)
        acc = torch.full_like(dst, NEG_INF) if cfirst[c] else dst.clone()
        for s in range(int(cstart[c]), int(cstart[c + 1])):
            acc = torch.logaddexp(acc, msg.view(-1, B, Ki)[int(items[s])])
        dst.copy_(acc)
    return out


def loo_down_product(type, cstart, cfold, cfirst, items, child, layer_fold, vals, der, val_off, n_child, H, Ki, Ko, B, dtype):
    """`ck_loo_down_product`: items are pairs (consumer global fold g, input position h).  Hadamard: unit k receives D_g[k] plus
    the values of the consumer's inputs h' != h at unit k.  Kronecker: unit i receives the log-sum-exp over the outputs o whose
    digit h is i of D_g[o] plus the values of the inputs h' != h at their digits of o."""
    vals, src = _c(vals, dtype), _c(der, dtype)
    out = src.clone()
    for c in range(n_child):
        dst = block(out, val_off, int(cfold[c]), B, Ki)
        acc = torch.full_like(dst, NEG_INF) if cfirst[c] else dst.clone()
        for s in range(int(cstart[c]), int(cstart[c + 1])):
            g, h = int(items[2 * s]), int(items[2 * s + 1])
            ch = child[(g - layer_fold) * H:(g - layer_fold + 1) * H]
            t = block(src, val_off, g, B, Ko)
            if type == HADAMARD:
                for h2 in range(H):
                    if h2 != h:
                        t = t + block(vals, val_off, int(ch[h2]), B, Ki)
            else:
                t = _kron_view(t, B, H, Ki)
                for h2 in range(H - 1, -1, -1):
                    if h2 != h:
                        shape = [B] + [1] * H
                        shape[h2 + 1] = Ki
                        t = t + block(vals, val_off, int(ch[h2]), B, Ki).reshape(shape)
                t = lse(t.movedim(h + 1, 1).reshape(B, Ki, -1), 2)
            acc = torch.logaddexp(acc, t)
        dst.copy_(acc)
    return out


def _loo_units(entries, a, b, der, val_off, B):
    """The derivatives (B, U) of the units of entries a .. b - 1, side by side, and max_k D_k over the finite ones."""
    d = torch.cat([block(der, val_off, int(entries[s][0]), B, int(entries[s][1])) for s in range(a, b)], dim=1)
    fin = torch.isfinite(d)
    mD = torch.where(fin, d, torch.full_like(d, NEG_INF)).amax(1, keepdim=True)
    return d, fin, mD


def loo_leaf_categorical(entries, qstart, Q, Cout, ntab, lz, der, val_off, bad, B, dtype):
    """`ck_loo_leaf_categorical`: out (B, Q, Cout) = a_c / sum_c' a_c', a_c = sum_k exp(D_k + log Z_k - shift) ntab[k, c];
    log Z_k = -inf drops the unit; NaN for a (row, variable) without mass and for a row with bad[n] != 0."""
    ntab, lz, der = _c(ntab, dtype), _c(lz, dtype), _c(der, dtype)
    out = torch.zeros(B, Q, Cout, dtype=torch_dtype(dtype))
    for q in range(Q):
        a, b = int(qstart[q]), int(qstart[q + 1])
        d, fin, mD = _loo_units(entries, a, b, der, val_off, B)
        z = torch.cat([lz[int(entries[s][4]):int(entries[s][4]) + int(entries[s][1])] for s in range(a, b)]).unsqueeze(0)
        keep = fin & (z > NEG_INF)
        t = torch.where(keep, (_zero_where(fin, d) - _zero_where(torch.isfinite(mD), mD)) + _zero_where(z > NEG_INF, z).expand_as(d),
                        torch.full_like(d, NEG_INF))
        m2 = t.amax(1, keepdim=True)
        pi = _zero_where(keep, torch.exp(_zero_where(keep, t) - _zero_where(torch.isfinite(m2), m2)))
        tab = torch.zeros(d.shape[1], Cout, dtype=torch_dtype(dtype))
        u = 0
        for s in range(a, b):
            _, K, C, off = (int(x) for x in entries[s][:4])
            c = min(C, Cout)
            tab[u:u + K, :c] = ntab[off:off + K * C].view(K, C)[:, :c]
            u += K
        ac = pi @ tab
        total = ac.sum(1, keepdim=True)
        out[:, q] = torch.where(total > 0, ac / torch.where(total > 0, total, torch.ones_like(total)), torch.full_like(ac, float("nan")))
    out[torch.as_tensor(bad) != 0] = float("nan")
    return out


def loo_leaf_gaussian(entries, qstart, Q, mean, stddev, der, val_off, bad, B, dtype):
    """`ck_loo_leaf_gaussian`: out (B, Q, 2) = (S1, S2 - S1^2) with pi = softmax_k(D_k) over the finite D_k."""
    mean, stddev, der = _c(mean, dtype), _c(stddev, dtype), _c(der, dtype)
    out = torch.zeros(B, Q, 2, dtype=torch_dtype(dtype))
    for q in range(Q):
        a, b = int(qstart[q]), int(qstart[q + 1])
        d, fin, mD = _loo_units(entries, a, b, der, val_off, B)
        mu = torch.cat([mean[int(entries[s][3]):int(entries[s][3]) + int(entries[s][1])] for s in range(a, b)])
        sd = torch.cat([stddev[int(entries[s][3]):int(entries[s][3]) + int(entries[s][1])] for s in range(a, b)])
        has = torch.isfinite(mD).squeeze(1)
        p = _zero_where(fin, torch.exp(_zero_where(fin, d) - _zero_where(torch.isfinite(mD), mD)))
        t0 = torch.where(has, p.sum(1), torch.ones_like(p[:, 0]))
        s1, s2 = (p @ mu) / t0, (p @ (sd * sd + mu * mu)) / t0
        out[:, q] = torch.stack([s1, s2 - s1 * s1], -1)
        out[~has, q] = float("nan")
    out[torch.as_tensor(bad) != 0] = float("nan")
    return out


def loo_log_probs(entries, vstart, vkind, D, lz, der, vals, val_off, ev, x_float, bad, B, dtype):
    """`ck_loo_log_probs`: out (B, D) = lse_k(d_k + v_k) - lse_k(d_k + log Z_k), d_k = D_k - max_k D_k.  0 where the row misses v or
    no entry covers it; NaN where the leave-one-out mass is 0 or bad[n] != 0; -inf where only the observed value has no mass."""
    lz, der, vals = _c(lz, dtype), _c(der, dtype), _c(vals, dtype)
    out = torch.zeros(B, D, dtype=torch_dtype(dtype))
    for v in range(D):
        a, b = int(vstart[v]), int(vstart[v + 1])
        if a == b:
            continue
        d, fin, mD = _loo_units(entries, a, b, der, val_off, B)
        val = torch.cat([block(vals, val_off, int(entries[s][0]), B, int(entries[s][1])) for s in range(a, b)], dim=1)
        z = torch.cat([lz[int(entries[s][4]):int(entries[s][4]) + int(entries[s][1])] for s in range(a, b)]).unsqueeze(0)
        dd = _zero_where(fin, d) - _zero_where(torch.isfinite(mD), mD)
        ninf = torch.full_like(d, NEG_INF)
        num, den = lse(torch.where(fin, dd + val, ninf), 1), lse(torch.where(fin, dd + z, ninf), 1)
        res = torch.where(torch.isfinite(den), torch.where(torch.isfinite(num), num - den, num), torch.full_like(num, float("nan")))
        out[:, v] = torch.where(observed(ev[:, v], x_float, int(vkind[v]) == 2), res, torch.zeros_like(res))
    out[torch.as_tensor(bad) != 0] = float("nan")
    return out


# ----------------------------------------------------------------------------------------- the batch-reduced flow pass
def stats_edge_sum(type, diag, child, w, F, H, Ki, Ko, M, vals, flow, val_off, fold_off, live, B, edge, dtype, small=False):
    """`ck_stats_edge_sum`: edge (F, Ko, M) += N[f, k, i] = sum over the live rows of f_k w[f, k, i] exp(e_i - v_k); an entry with
    w <= 0 adds exactly 0, a unit with f_k = 0 or a v_k that is not finite drops out; mixing: block diagonals only.  The fp32
    runs take every term as a[n, k] w[k, i] g[n, i], a = f_k exp(-v_k - m), g = exp(e_i + m); a row with an entry of
    e_i + m >= 40 takes f_k exp(e_i - v_k) unshifted.  `small` (fp64): only the terms whose shifted factor is below SMALL."""
    vals, flow, w = _c(vals, dtype), _c(flow, dtype), _c(w, dtype).view(F, Ko, M)
    out = _c(edge, dtype).clone().view(F, Ko, M)
    live_t = torch.as_tensor(live) != 0
    for f in range(F):
        g_ = fold_off + f
        fk, vk = block(flow, val_off, g_, B, Ko), block(vals, val_off, g_, B, Ko)
        a, m, ok = flow_factors(fk, vk, dtype)
        e = entry_values(type, child[f * H:(f + 1) * H], H, Ki, vals, val_off, B)
        efin = e > NEG_INF
        has = torch.isfinite(m) & live_t.unsqueeze(1)
        ms = _zero_where(torch.isfinite(m), m)
        es = _zero_where(efin, e)
        if dtype == torch.float64:
            if small:
                a = _zero_where(a < SMALL, a)
            gg = _zero_where(efin & has, torch.exp(es + ms))
            N = _zero_where(has, a).t() @ gg
        else:
            slow = ((efin & (es + ms >= SLOW_SHIFT)).any(1, keepdim=True)) & has
            fact = has & ~slow
            gg = _zero_where(efin & fact, mul_exp(torch.ones_like(es), es, ms.expand_as(es), dtype))
            N = _zero_where(fact, a).t() @ gg
            rows = torch.nonzero(slow.squeeze(1)).flatten()
            if len(rows):  # f_k exp(e_i - v_k), no shift
                fs, vs_, er, okr = fk[rows], _zero_where(ok[rows], vk[rows]), es[rows], ok[rows]
                t = mul_exp(fs.unsqueeze(2).expand(-1, -1, M), er.unsqueeze(1).expand(-1, Ko, -1), -vs_.unsqueeze(2).expand(-1, -1, M), dtype)
                N = N + _zero_where(okr.unsqueeze(2) & efin[rows].unsqueeze(1), t).sum(0)
        add = _zero_where(w[f] > 0, w[f] * N)
        if diag:
            i = torch.arange(M)
            keep = torch.zeros(Ko, M, dtype=torch.bool)
            keep[i % Ki, i] = True
            add = _zero_where(keep, add)
        out[f] += add
    return out


def stats_leaf_categorical(scope, ntab, F, K, C, ev, x_float, D, flow, val_off, fold_off, live, B, leaf, dtype):
    """`ck_stats_leaf_categorical`: leaf (F, K, C) += over the live rows f_k at the state a row observes (nothing for a state at
    or beyond C), f_k ntab[f, k, c] at every state where the row misses the variable."""
    flow, ntab = _c(flow, dtype), _c(ntab, dtype).view(F, K, C)
    out = _c(leaf, dtype).clone().view(F, K, C)
    live_t = torch.as_tensor(live) != 0
    for f in range(F):
        fr = block(flow, val_off, fold_off + f, B, K)
        x = ev[:, int(scope[f])]
        obs = observed(x, x_float)
        c = x.to(torch.int64)
        hit = live_t & obs & (c < C)
        onehot = torch.zeros(B, C, dtype=torch_dtype(dtype))
        onehot[hit, c[hit]] = 1
        miss = _zero_where((live_t & ~obs).unsqueeze(1), fr).sum(0)
        out[f] += fr.t() @ onehot + miss.unsqueeze(1) * ntab[f]
    return out


def stats_leaf_gaussian(scope, mean, stddev, F, K, ev, D, flow, val_off, fold_off, live, B, leaf, dtype):
    """`ck_stats_leaf_gaussian`: leaf (F, K, 3) += (sum f_k, sum f_k m1, sum f_k m2) over the live rows, (m1, m2) = (x, x^2)
    where the row observes the variable, (mean_k, stddev_k^2 + mean_k^2) where it is missing (NaN)."""
    flow, mean, stddev, ev = _c(flow, dtype), _c(mean, dtype).view(F, K), _c(stddev, dtype).view(F, K), _c(ev, dtype)
    out = _c(leaf, dtype).clone().view(F, K, 3)
    live_t = torch.as_tensor(live) != 0
    for f in range(F):
        fr = _zero_where(live_t.unsqueeze(1), block(flow, val_off, fold_off + f, B, K))
        x = ev[:, int(scope[f])].unsqueeze(1)
        obs = ~torch.isnan(x)
        xs = _zero_where(obs, x)
        m1 = torch.where(obs, xs.expand(B, K), mean[f].expand(B, K))
        m2 = torch.where(obs, (xs * xs).expand(B, K), (stddev[f] * stddev[f] + mean[f] * mean[f]).expand(B, K))
        out[f] += torch.stack([fr.sum(0), (fr * m1).sum(0), (fr * m2).sum(0)], -1)
    return out


def stats_unit_sum(flow, val_off, fold_ko, unit_off, total_folds, live, B, unit, dtype):
    """`ck_stats_unit_sum`: unit[unit_off[g] + k] += the sum of f_k over the live rows, for every global fold g."""
    flow = _c(flow, dtype)
    out = _c(unit, dtype).clone()
    live_t = torch.as_tensor(live) != 0
    for g in range(total_folds):
        K, o = int(fold_ko[g]), int(unit_off[g])
        out[o:o + K] += _zero_where(live_t.unsqueeze(1), block(flow, val_off, g, B, K)).sum(0)
    return out


# ------------------------------------------------------------------------------------------------- tables of the tests
def message_csr(type, child, F, H, flow_pass, cfolds):
    """The CSR lists of the segment launch that follows a down-sum launch: for every child fold of `cfolds`, the message slots
    that target it, in slot order (a fold named twice by one consumer receives two items)."""
    cstart, items = [0], []
    for c in cfolds:
        for f in range(F):
            for h in range(2 if type == TUCKER else H):
                if int(child[f * H + h]) == int(c):
                    items.append({SUM: f * H + h, CPT: f if flow_pass else f * H + h, TUCKER: 2 * f + h}[type])
        cstart.append(len(items))
    return np.array(cstart, dtype=np.int32), np.array(items, dtype=np.int32)


def forward_values(type, child, w, F, H, Ki, Ko, M, vals, val_off, fold_off, B):
    """The (F, B, Ko) log values of a sum-type layer over the child blocks of the fp64 arena `vals`: v_k = log sum_i w[k, i]
    exp(e_i), -inf where the sum is 0 (mixing: pass the weight with zeros off its block diagonals)."""
    out = []
    for f in range(F):
        e = entry_values(type, child[f * H:(f + 1) * H], H, Ki, vals, val_off, B)
        wf = w.view(F, Ko, M)[f].double()
        lw = torch.where(wf > 0, torch.log(torch.where(wf > 0, wf, torch.ones_like(wf))), torch.full_like(wf, NEG_INF))
        out.append(lse(e.unsqueeze(1) + lw.unsqueeze(0), 2))
    return torch.stack(out)


def arena_offsets(sizes, gap=64):
    """Word offsets of blocks of `sizes` words with `gap` words in front of, between and behind them, every offset a multiple
    of 4 words (the layout of guarded_buffers._GuardedArena), and the total."""
    at, off = gap, []
    for n in sizes:
        off.append(at)
        at = (at + int(n) + 3) // 4 * 4 + gap
    return off, at


FAMILIES = ["normal", "far-tail", "spread", "dropped", "dead-row", "wzero"]


def touches_unit0(type, H, Ki, M):
    """The entries that read unit 0 of some input."""
    i = torch.arange(M)
    if type == SUM:
        return i % Ki == 0
    if type == CPT:
        return i == 0
    return (i // Ki == 0) | (i % Ki == 0)


class SumCase:
    """One launch of a sum-type layer with a consistent forward: global folds = `fold_off` child folds (or, with fold_off = 0,
    the F parent folds first), the parents' values v = log sum_i w exp(e_i) formed in fp64 from the fp32 children and weights and
    rounded once.  `flow_pass`: the parents' arena blocks hold flows f in [0, 1], else log derivatives D = log f - v.  Families:
    'normal'; 'far-tail' (entry values around -700); 'spread' (entries, unit weights and flows each spread over e^30); 'dropped'
    (30 % of the units f = 0 / D = -inf, unit 1 of every fold without weights, so v = -inf, 10 % of the child values -inf);
    'dead-row' (rows 0 and B // 2: every unit dropped); 'wzero' (unit 0 the heaviest of every row and without weight on entry
    0, the last entry without any weight, 10 % zeros); 'over80' / 'over80e' / 'kslow' (see `_shift_family`)."""

    def __init__(self, type, diag, F, H, Ki, Ko, B, fam, g, fold_off=0, flow_pass=True):
        self.type, self.diag, self.F, self.H, self.Ki, self.Ko, self.B, self.fam, self.flow_pass = type, diag, F, H, Ki, Ko, B, fam, flow_pass
        M = self.M = H * Ki if type == SUM else (Ki if type == CPT else Ki * Ki)
        nc = self.nc = min(3, F * H)
        assert fold_off in (0, nc)
        self.fold_off = fold_off
        cbase = 0 if fold_off else F
        self.cfolds = list(range(cbase, cbase + nc))
        self.pfolds = list(range(fold_off, fold_off + F))
        self.child = np.array([cbase + (f * H + h) % nc for f in range(F) for h in range(H)], dtype=np.int32)
        sizes = [0] * (F + nc)
        for c in self.cfolds:
            sizes[c] = B * Ki
        for p in self.pfolds:
            sizes[p] = B * Ko
        self.sizes = sizes
        self.val_off, self.words = arena_offsets(sizes)
        self.val_off = np.array(self.val_off, dtype=np.int64)
        nan = float("nan")
        hdiv = {SUM: 1, CPT: H, TUCKER: 2}[type]
        # children
        cv = torch.randn(nc, B, Ki, generator=g) * 2
        if fam == "far-tail":
            cv = torch.round((cv - 700.0 / hdiv) * 1024) / 1024  # (multiples of 2^-10: the entry values, sums of up to 3, are exact in fp32)
        elif fam == "spread":
            cv = (torch.rand(nc, B, Ki, generator=g) * 60 - 30) / hdiv
        elif fam == "dropped" and Ki > 1:
            cv[torch.rand(nc, B, Ki, generator=g) < 0.1] = NEG_INF
        # weights
        w = torch.softmax(torch.randn(F, Ko, M, generator=g), -1)
        f = torch.rand(F, B, Ko, generator=g) * 0.999 + 0.001
        if fam == "spread":
            w = w * torch.exp(torch.rand(F, Ko, 1, generator=g) * 30 - 15)
            f = torch.exp(-30 * torch.rand(F, B, Ko, generator=g))
        if fam == "dropped":
            f[torch.rand(F, B, Ko, generator=g) < 0.3] = 0.0
            if Ko > 2:
                w[:, 1, :] = 0.0
        if fam == "dead-row":
            f[:, 0] = 0.0
            f[:, B // 2] = 0.0
        if fam == "wzero":
            w[torch.rand(F, Ko, M, generator=g) < 0.1] = 0.0
            if M > 1:
                w[:, :, M - 1] = 0.0
                w[:, 0, :] *= 1e-3
                w[:, 0, 0] = 0.0
                f = f * 1e-3
                f[:, :, 0] = 1.0
        if fam in ("over80", "over80e", "kslow"):
            cv, w, f = self._shift_family(cv, w, f, g, hdiv)
        self.mask = None
        if diag:
            i = torch.arange(M)
            self.mask = torch.zeros(Ko, M, dtype=torch.bool)
            self.mask[i % Ki, i] = True
        self.w = w.contiguous()
        vals = torch.full((self.words,), nan)
        for j, c in enumerate(self.cfolds):
            block(vals, self.val_off, c, B, Ki).copy_(cv[j])
        wfwd = self.w if not diag else torch.where(self.mask, self.w, torch.zeros_like(self.w))
        v = forward_values(type, self.child, wfwd, F, H, Ki, Ko, M, vals.double(), self.val_off, 0, B).float()
        for j, p in enumerate(self.pfolds):
            block(vals, self.val_off, p, B, Ko).copy_(v[j])
        self.vals = vals
        # the parents' arena blocks, and a prior in every child block
        arena = torch.full((self.words,), nan)
        shift = -cv.amax(-1, keepdim=True)  # (the size of a derivative of a child: about minus its value)
        shift = torch.where(torch.isfinite(shift), shift, torch.zeros_like(shift))
        prior = torch.rand(nc, B, Ki, generator=g) if flow_pass else torch.randn(nc, B, Ki, generator=g) + shift
        for j, c in enumerate(self.cfolds):
            block(arena, self.val_off, c, B, Ki).copy_(prior[j])
        if not flow_pass:
            pos = f > 0
            d = torch.where(torch.isfinite(v), torch.log(torch.where(pos, f, torch.ones_like(f))) - v, torch.randn(F, B, Ko, generator=g))
            f = torch.where(pos, d, torch.full_like(d, NEG_INF))
        for j, p in enumerate(self.pfolds):
            block(arena, self.val_off, p, B, Ko).copy_(f[j])
        self.arena = arena

    def _shift_family(self, cv, w, f, g, hdiv):
        """'over80' and 'over80e' put the two exponents of the flow pass, -v_k - m and m + e_i, on both sides of 80, 'kslow'
        e_i + m of ck_stats_edge_sum on both sides of 40, with every fp64 flow and statistic at most 1 (a message of several
        units: their number).
        'over80': the odd units' weights lie e^-80 below the even units' (e^20 and e^-60 times a softmax row) and their flows
        at e^-74 .. e^-83, so that both kinds of unit are about as heavy and -v_k - m of the odd ones is about 76 .. 83.
        'over80e' / 'kslow': unit 0 of every child block lies delta(n) / hdiv above the others, delta in [76, 81] / [35, 46].
        Unit 0 of the fold is the heaviest of the row, f = 1, and has no weight on the entries that read a unit 0; the other
        units have their weight there and carry f in [0.2, 0.4]: their values lie about delta above unit 0's, so m is about
        minus the plain entry values, e_i + m about delta on the raised entries, the factors of these units about e^-delta (a
        normal fp32 number: delta < 83) and what the raised entries receive at most f."""
        F, Ko, M, B, Ki = self.F, self.Ko, self.M, self.B, self.Ki
        assert Ki > 1 and Ko > 1
        if self.fam == "over80":
            w[:, 0::2] *= float(np.exp(20.0))
            w[:, 1::2] *= float(np.exp(-60.0))
            f[:, :, 1::2] = torch.exp(-(74 + 9 * torch.rand(F, B, Ko // 2, generator=g)))
            return cv, w, f
        lo, hi = (76.0, 81.0) if self.fam == "over80e" else (35.0, 46.0)
        delta = lo + (hi - lo) * torch.rand(1, B, 1, generator=g)
        cv = cv.clone()
        cv[:, :, :1] += delta / hdiv
        w[:, 0, touches_unit0(self.type, self.H, Ki, M)] = 0.0
        f[:, :, 1:] = 0.2 + 0.2 * torch.rand(F, B, Ko - 1, generator=g)
        f[:, :, 0] = 1.0
        return cv, w, f

    def csr(self, cfirst):
        """(cstart, cfold, cfirst, items) of the segment launch after this launch's down-sum."""
        cstart, items = message_csr(self.type, self.child, self.F, self.H, self.flow_pass, self.cfolds)
        return cstart, np.array(self.cfolds, dtype=np.int32), np.array(cfirst, dtype=np.int32), items
