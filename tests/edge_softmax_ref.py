"""fp64 segment softmax of head-major per-edge scores over the rows of a CSR (checker side only; on the scores' device).  Shared by
test_edge_attention_gpu.py and test_ops_layouts_gpu.py."""
import torch

SOFTMAX_RTOL = 1e-5     # of max(1, |ref|) for the probabilities, of max(1, sum of |terms|) for the gradient (test_bindings_agree_gpu.py too)


def _rows_of(rp):
    rp = rp.long()
    return torch.repeat_interleave(torch.arange(rp.numel() - 1, device=rp.device), rp[1:] - rp[:-1])


def _softmax64(s, rp):
    """fp64 segment softmax of head-major scores s [H, nnz] over the rows of rp."""
    rows = _rows_of(rp.to(s.device))
    n = rp.numel() - 1
    s = s.double()
    m = torch.full((s.shape[0], n), -float("inf"), dtype=torch.float64, device=s.device)
    m = m.scatter_reduce(1, rows.expand_as(s), s, reduce="amax")
    ex = torch.exp(s - m[:, rows])
    den = torch.zeros(s.shape[0], n, dtype=torch.float64, device=s.device).index_add_(1, rows, ex)
    return ex / den[:, rows]
