"""Structure learning: the Chow-Liu tree of tabular data ("Structure learning").

The reference's ``ChowLiuTree`` (cirkit/templates/region_graph/algorithms/chow_liu.py:11-254): pairwise mutual information,
maximum spanning tree, rooted at the vertex of least eccentricity.  Two paths to the (D, D) matrix:

* categorical data on a ROCm device -- `pairwise_mutual_information`: the joint counts are the Gram matrix of the one-hot
  encoding, formed tile by tile on the bf16 matrix pipe and reduced to mutual information in fp64 in the kernel's epilogue
  (cirkit_amd/csrc/ck_mi.hip); the reference's (D, D, C^2) count tensor is never written;
* everything else (Gaussian and mixed columns, categorical data on the CPU) -- the reference's own formulas with torch on
  the CPU, in fp32 like the reference, so that near-ties between edges resolve as they do there.

Both end in the same scipy.sparse.csgraph calls as the reference, on the host.  `templates.tabular_data('chow-liu-tree',
data=...)` turns the tree into a hidden Chow-Liu tree region graph (`templates.tree_to_region_graph`) and a plan.
"""

from __future__ import annotations

import numpy as np

from . import _capi as capi


# ---------------------------------------------------------------------------------------------
# the device path: categorical data
# ---------------------------------------------------------------------------------------------
def _check_rows(data) -> None:
    if data.ndim != 2:
        raise ValueError("structure learning needs tabular data (rows x features)")
    if data.shape[0] < 1 or data.shape[1] < 1:
        raise ValueError(f"structure learning needs at least one row and one feature, got {tuple(data.shape)}")
    if data.shape[0] > capi.CK_MI_MAX_ROWS:  # on the shape alone: before anything is allocated
        raise ValueError(f"{data.shape[0]} rows: the pair counts are accumulated in fp32, exact up to 2^24 rows")


class _Staged:
    """The column-major uint8 copy of a batch (one variable's codes contiguous along n), validated."""

    def __init__(self, data, num_categories: int | None, num_bins: int | None) -> None:
        import torch

        _check_rows(data)
        if not isinstance(data, torch.Tensor) or data.device.type != "cuda":
            raise ValueError("the pairwise counts run on a ROCm device: pass a tensor that lives on one "
                             "(chow_liu_predecessors takes data on the CPU through the host path)")
        if data.dtype not in (torch.int64, torch.int32):
            if data.dtype.is_floating_point or data.dtype == torch.bool or data.dtype.is_complex:
                raise ValueError(f"categorical data must be integers, got {data.dtype}")
            data = data.to(torch.int64)
        if num_bins is not None and num_categories is None:
            raise ValueError("Number of categories must be known if rescaling in bins")
        self.N, self.D = int(data.shape[0]), int(data.shape[1])
        c_in = int(data.max().item()) + 1 if num_categories is None else int(num_categories)
        if c_in < 1:
            raise ValueError("negative entry in categorical data" if num_categories is None
                             else f"num_categories = {num_categories}")
        if c_in > capi.CK_MI_MAX_STATES:
            raise ValueError(f"{c_in} states: at most {capi.CK_MI_MAX_STATES} (rescale ordinal features with num_bins)")
        div = 1
        if num_bins is not None:
            if not 1 <= num_bins <= c_in:
                raise ValueError(f"num_bins = {num_bins} with {c_in} categories")
            div = c_in // num_bins
        self.C = (c_in - 1) // div + 1  # the states x // div can take
        self.ldn = (self.N + 15) // 16 * 16
        self.device = data.device
        data = data.contiguous()
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream(self.device).cuda_stream
            self.codes = torch.zeros((self.D, self.ldn), dtype=torch.uint8, device=self.device)
            bad = torch.zeros(1, dtype=torch.int32, device=self.device)
            capi.call("ck_mi_stage", data.data_ptr(), int(data.dtype == torch.int64), self.N, self.D, c_in, div,
                      self.codes.data_ptr(), self.ldn, bad.data_ptr(), self.stream)
            if int(bad.item()):
                raise ValueError(f"categorical data holds an entry outside 0 .. {c_in - 1}")


def pairwise_mutual_information(data, num_categories: int | None = None, *, alpha: float = 0.01, num_bins: int | None = None):
    """(D, D) float64 mutual information of the integer columns of `data` (a tensor on a ROCm device) with Laplace smoothing
    `alpha`, as `_categorical_mutual_info` of the reference defines it: joint = (count + alpha) / (N + C^2 alpha), marginal =
    (count + C alpha) / (N + C^2 alpha), MI[i, j] = sum_ab joint (log joint - log marginal_i(a) marginal_j(b)), diagonal 0.
    Exactly symmetric, and bitwise repeatable.  `num_categories=None` takes max + 1; `num_bins` rescales ordinal codes
    (x // (num_categories // num_bins)) and the rescaled data has as many states as that division leaves."""
    import torch

    st = _Staged(data, num_categories, num_bins)
    if not alpha > 0.0:
        raise ValueError(f"the smoothing alpha must be positive, got {alpha}")
    with torch.cuda.device(st.device):
        logm = torch.empty((st.D, st.C), dtype=torch.float64, device=st.device)
        mi = torch.zeros((st.D, st.D), dtype=torch.float64, device=st.device)
        capi.call("ck_mi_marginals", st.codes.data_ptr(), st.N, st.D, st.ldn, st.C, float(alpha), None, logm.data_ptr(), st.stream)
        capi.call("ck_mi_pairs", st.codes.data_ptr(), st.N, st.D, st.ldn, st.C, float(alpha), logm.data_ptr(), mi.data_ptr(), None,
                  st.stream)
    return mi


def pairwise_counts(data, num_categories: int | None = None, *, num_bins: int | None = None):
    """(D, D, C, C) int64 joint counts, counts[i, j, a, b] = #{n : x[n, i] = a, x[n, j] = b}: the kernel of
    `pairwise_mutual_information` with an epilogue that stores its tiles.  At most 2^28 elements."""
    import torch

    st = _Staged(data, num_categories, num_bins)
    if st.D * st.D * st.C * st.C > capi.CK_MI_MAX_COUNTS:
        raise ValueError(f"{st.D}^2 x {st.C}^2 joint counts exceed 2^28 elements; pairwise_mutual_information does not store them")
    with torch.cuda.device(st.device):
        counts = torch.empty((st.D, st.D, st.C, st.C), dtype=torch.int64, device=st.device)
        capi.call("ck_mi_pairs", st.codes.data_ptr(), st.N, st.D, st.ldn, st.C, 0.0, None, None, counts.data_ptr(), st.stream)
    return counts


# ---------------------------------------------------------------------------------------------
# the host path: the reference's formulas with torch on the CPU
# ---------------------------------------------------------------------------------------------
def _categorical_mutual_information(data, num_categories: int | None, chunk_size: int | None, alpha: float = 0.01):
    """Pairwise mutual information of integer columns with Laplace smoothing `alpha` (chow_liu.py:107-151):
    joint counts of every pair of columns, the marginals read off the diagonal blocks, and
    MI[i, j] = sum_kl P_ij(k, l) (log P_ij(k, l) - log P_i(k) P_j(l)), diagonal set to 0.
    Evaluated with torch in fp32 like the reference, so that near-ties between edges resolve the same way."""
    import torch

    x = torch.as_tensor(data).long()
    n, d = x.shape
    c = int(x.max().item() + 1) if num_categories is None else int(num_categories)
    counts = torch.zeros((d, d, c * c), dtype=torch.long)
    for part in x.split(n if chunk_size is None else chunk_size):
        pair = part.t().unsqueeze(1) * c + part.t().unsqueeze(0)  # (d, d, rows): category pair of columns (i, j)
        counts.scatter_add_(-1, pair, torch.ones_like(pair))
    counts = counts.view(d, d, c, c)
    diag = torch.arange(d)
    cats = torch.arange(c)
    marg_counts = counts[diag, diag][:, cats, cats]  # (d, c): a column paired with itself counts its categories
    denom = n + c * c * alpha
    marg = (marg_counts + c * alpha) / denom
    joint = (counts + alpha) / denom
    joint[diag, diag] = torch.diag_embed(marg)
    indep = torch.einsum("ik,jl->ijkl", marg, marg)
    return (joint * (joint.log() - indep.log())).sum(dim=(2, 3)).fill_diagonal_(0)


def _mixed_mutual_information(data, is_categorical: list[bool], normalize: bool = True):
    """Mutual information between columns of mixed type (chow_liu.py:154-254): Gaussian columns among themselves
    as a multivariate normal, categorical columns among themselves by counting, a Gaussian column C against a
    categorical column D as H(C) - sum_d p(d) H(C | D = d) with Gaussian entropies (variance + 1e-4); optionally
    normalised by the column entropies, NMI = 2 I / (H_i + H_j)."""
    import torch

    x = torch.as_tensor(data)
    mask = torch.tensor(is_categorical, dtype=torch.bool)
    cont = torch.where(~mask)[0]
    disc = torch.where(mask)[0]
    d = x.shape[1]
    mi = torch.zeros((d, d), dtype=torch.float32)
    if len(cont) > 1:
        r = torch.corrcoef(x[:, cont].t()).fill_diagonal_(0)
        mi[cont.unsqueeze(1), cont] = (-0.5 * torch.log(1 - r**2)).float()
    if len(disc) > 1:
        mi[disc.unsqueeze(1), disc] = _categorical_mutual_information(x[:, disc].long(), None, None).float()

    def h_gauss(col):
        return 0.5 * (torch.log(2 * torch.pi * torch.var(col, unbiased=False) + 1e-4) + 1)

    ncat = {j: int(x[:, j].max() + 1) for j in disc.tolist()}
    p_d = {j: x[:, j].long().bincount(minlength=ncat[j]).float() / x.shape[0] for j in disc.tolist()}
    h_c = {i: h_gauss(x[:, i]) for i in cont.tolist()}
    for i in cont.tolist():
        for j in disc.tolist():
            cond = torch.stack([h_gauss(x[:, i][x[:, j] == k]) for k in range(ncat[j])], dim=0)
            mi[i, j] = mi[j, i] = h_c[i] - torch.sum(cond * p_d[j])
    if normalize:
        ent = torch.zeros(d, dtype=torch.float32)
        ent[cont] = torch.tensor(list(h_c.values()), dtype=torch.float32)
        ent[disc] = torch.tensor([-(p.log() * p).sum() for p in p_d.values()], dtype=torch.float32)
        mi = 2 * mi / (ent.unsqueeze(0) + ent.unsqueeze(1))
    return mi.fill_diagonal_(0)


def _on_device(x) -> bool:
    import torch

    return isinstance(x, torch.Tensor) and x.device.type == "cuda"


def chow_liu_predecessors(data, input_type: str | list[str], *, root: int | None = None, chunk_size: int | None = None,
                          num_categories: int | None = None, num_bins: int | None = None) -> np.ndarray:
    """The Chow-Liu tree of tabular `data` (rows x features) as a list of predecessors (-1 at the root): maximum
    spanning tree of the pairwise mutual information, rooted at `root` or at the vertex of least eccentricity
    (chow_liu.py:11-104).  Uses the same scipy.sparse.csgraph routines as the reference.  Categorical data that lives on a
    ROCm device goes through `pairwise_mutual_information`; everything else through the reference's formulas on the CPU."""
    import torch
    from scipy.sparse import csgraph

    x = torch.as_tensor(data)
    if x.ndim != 2:
        raise ValueError("Chow-Liu structure learning needs tabular data (rows x features)")
    if root is not None and not 0 <= root < x.shape[1]:
        raise ValueError("the root must be one of the features")
    if isinstance(input_type, list):
        mi = _mixed_mutual_information(x.cpu(), [t == "categorical" for t in input_type])
    elif input_type == "categorical":
        if num_bins is not None and num_categories is None:
            raise ValueError("Number of categories must be known if rescaling in bins")
        if _on_device(x):
            mi = pairwise_mutual_information(x, num_categories, num_bins=num_bins)
        else:
            if num_bins is not None:
                x = torch.div(x, num_categories // num_bins, rounding_mode="floor")
            mi = _categorical_mutual_information(x.long(), num_categories, chunk_size)
    elif input_type == "gaussian":
        x = x.cpu()
        mi = -0.5 * torch.log(1 - torch.corrcoef(x.t()) ** 2)
    else:
        raise NotImplementedError(f"MI computation not implemented for {input_type} input units")
    mst = csgraph.minimum_spanning_tree(-(mi.cpu().numpy() + 1.0), overwrite=True)
    if root is None:
        dist = csgraph.dijkstra(abs(mst).todense(), directed=False, return_predecessors=False)
        root = int(np.argmin(np.max(dist, axis=1)))
    _, pred = csgraph.breadth_first_order(mst, directed=False, i_start=root, return_predecessors=True)
    pred[root] = -1
    return pred
