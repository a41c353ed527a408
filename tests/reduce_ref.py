"""fp64 torch restatement of the max / min / mean over every row's neighbours (checker side only; on the CPU): scatter_reduce over
X[column_index].  torch splits the gradient of a tied extreme evenly and the library sends it to the edge earliest in column_index:
``_no_ties`` tells whether an input has such a tie, ``first_edge_routing`` is the library's rule written out.  Shared by
test_reduce_ops_gpu.py, test_pna_ops_gpu.py and test_ops_layouts_gpu.py."""
import torch


def _rows_of(rp):
    rp = rp.long()
    return torch.repeat_interleave(torch.arange(rp.numel() - 1), rp[1:] - rp[:-1])


def _agg64(X, rp, ci, how):
    """fp64 reference on the CPU: scatter_reduce over X[column_index] with include_self=False; rows without edges give 0."""
    rows = _rows_of(rp)
    n = rp.numel() - 1
    src = X[ci.long()]
    out = torch.zeros(n, X.shape[1], dtype=X.dtype)
    return out.scatter_reduce(0, rows[:, None].expand_as(src), src, reduce=how, include_self=False)


def _no_ties(X, rp, ci, how):
    """No row of the reference has its extreme twice in a column."""
    ext = _agg64(X, rp, ci, how)
    rows = _rows_of(rp)
    hits = torch.zeros_like(ext).index_add_(0, rows, (X[ci.long()] == ext[rows]).to(X.dtype))
    return bool((hits <= 1).all())


def first_edge_routing(X, rows, src, n_out, how, G):
    """(extreme [n_out, F], dX [n_in, F]) with the library's tie rule: of the edges of row i whose source holds the extreme of
    column f, the one earliest in column_index receives all of G[i, f] (torch's scatter_reduce splits it evenly among them).
    rows / src: int64 [nnz] in CSR order; X [n_in, F], G [n_out, F], any float dtype; a row without edges gives 0 and routes
    nothing.  Without a tie this is the gradient of ``_agg64``."""
    S = X[src]
    idx = rows[:, None].expand_as(S)
    ext = torch.zeros(n_out, X.shape[1], dtype=X.dtype, device=X.device).scatter_reduce(0, idx, S, reduce=how, include_self=False)
    pos = torch.arange(src.numel(), device=X.device)[:, None].expand_as(S)
    hit = S == ext[rows]
    cand = torch.where(hit, pos, torch.full_like(pos, src.numel()))
    first = torch.full((n_out, X.shape[1]), src.numel(), dtype=torch.int64, device=X.device).scatter_reduce(0, idx, cand, reduce="amin",
                                                                                                           include_self=True)
    wins = hit & (pos == first[rows])
    dX = torch.zeros_like(X).index_add_(0, src, torch.where(wins, G[rows], torch.zeros_like(S)))
    return ext, dX
