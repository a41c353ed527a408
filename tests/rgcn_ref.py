"""fp64 dense restatement of the relation-typed aggregation and of an R-GCN layer in basis form (checker side only): one
[num_dst, num_src] matrix per relation, A_r[i, j] = sum of the factors n[e] of the edges i <- j of type r; T[:, b] = sum_r coef[r, b]
A_r X and Y = T V + X_dst W_self + bias.  Differentiable by torch autograd; shared by test_rgcn_ops_gpu.py and
test_ops_layouts_gpu.py."""
import torch


def dense_relations(rp, ci, ety, nrm, R, n_dst, n_src):
    """float64 [R, n_dst, n_src] on the GPU."""
    rp, ci, ety = (torch.as_tensor(a).cpu().long() for a in (rp, ci, ety))
    rows = torch.repeat_interleave(torch.arange(n_dst), rp[1:] - rp[:-1])
    w = torch.ones(len(ci), dtype=torch.float64) if nrm is None else torch.as_tensor(nrm).cpu().double()
    A = torch.zeros(R, n_dst, n_src, dtype=torch.float64)
    A.index_put_((ety, rows, ci), w, accumulate=True)
    return A.cuda()


def dense_expand(A, X, coef):
    AX = torch.einsum("rij,jf->rif", A, X)
    return torch.einsum("rb,rif->ibf", coef, AX).reshape(A.shape[1], -1)


def dense_layer(A, X, coef, V, W_self, bias):
    return dense_expand(A, X, coef) @ V.reshape(-1, V.shape[2]) + X[:A.shape[1]] @ W_self + bias
