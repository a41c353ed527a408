"""Graph classification on batches of small graphs: conv layers, a readout, a linear layer.

    python -m gnnadvisor_osdi21_amd.graph_main --model gin --num_graphs 4096 --graph_nodes 8,72 --batch_graphs 256 --readout sum
    python -m gnnadvisor_osdi21_amd.graph_main --model gine --edge_dim 4 --num_graphs 4096 --batch_graphs 256
    python -m gnnadvisor_osdi21_amd.graph_main --model schnet --cutoff 1.5 --num_graphs 4096 --batch_graphs 256

The reference evaluates half of its inputs ("Type II": collections of small graphs) with node-level drivers only; this driver
finishes such a model inside the library.  A seeded synthetic collection (graph.small_graphs) is kept on the device as a
batching.GraphDataset; every step cuts a mini-batch of ``--batch_graphs`` graphs out of it (GraphDataset.batch), runs two or more
GCN / GIN layers on the block-diagonal CSR (with ``--norm graph`` an ops.GraphNorm between every conv layer and its ReLU; with ``--pool topk|sag`` a pooling layer after every conv layer but the last keeps
the best-scoring ``--pool_ratio`` of the nodes of every graph and the next layer runs on the coarsened batch), reduces the node
rows of every graph to one row (ops.Readout, one fused call for all
the statistics of ``--readout``; with ``--attention_readout scalar|channel`` an ops.AttentionalReadout next to them), and trains
a per-graph classifier.  Prints ``Time (ms): %.3f`` per epoch as main.py does.
The label of a graph is a function of its size and its features' mean, so that the loss has something to learn.
``--model gine --edge_dim K`` draws K features per edge (not symmetrised: e_ij != e_ji), lets the label depend on them too, and
trains edgeconv.GINEConv layers on mini-batches built as ``directed`` ones, so that the backward finds an edge's features through
the device-built ``perm`` of the transposed batch; with ``--pool`` the edge features follow the coarsening.
``--model schnet --cutoff R [--max_neighbors K]`` draws point sets instead (graph.small_point_clouds: the label is the class of a
set's mean pairwise distance) and builds the graph of every mini-batch on the device from the batch's positions at every step
(spatial.radius_graph: libgnna gnna_radius_graph_f32; ``--fused_graph False`` composes it from torch ops), runs
spatial.SchNetInteraction layers on it and the same readout.
"""
import argparse
import sys
import time

import torch


def _bool(text):
    if text not in ("True", "False"):
        raise argparse.ArgumentTypeError("expected True or False (got %r)" % text)
    return text == "True"


def build_parser():
    p = argparse.ArgumentParser(description="graph classification on batches of small graphs")
    p.add_argument("--model", type=str, default="gin", help="gcn, gin, or gine (GIN with edge features: needs --edge_dim)")
    p.add_argument("--edge_dim", type=int, default=0, help="--model gine: features per edge of the synthetic collection")
    p.add_argument("--fused_edge", type=_bool, default=True, help="False: the edge-feature aggregation composed from torch ops")
    p.add_argument("--cutoff", type=float, default=None, help="--model schnet: the radius of the graph built from the positions")
    p.add_argument("--max_neighbors", type=int, default=None, help="--model schnet: keep the nearest K (1 .. 64) within the cutoff")
    p.add_argument("--num_gaussians", type=int, default=32, help="--model schnet: centres of the distance expansion")
    p.add_argument("--fused_graph", type=_bool, default=True, help="False: the radius graph composed from torch ops")
    p.add_argument("--density", type=float, default=1.0, help="--model schnet: points per unit volume of the synthetic point sets")
    p.add_argument("--num_graphs", type=int, default=4096, help="graphs in the synthetic collection")
    p.add_argument("--graph_nodes", type=str, default="8,72", help="MIN,MAX nodes per graph")
    p.add_argument("--avg_degree", type=float, default=4.0, help="average degree inside a graph")
    p.add_argument("--batch_graphs", type=int, default=256, help="graphs per mini-batch")
    p.add_argument("--readout", type=str, default="sum", help="comma list of sum, mean, max, min")
    p.add_argument("--attention_readout", type=str, default="none",
                   help="none, scalar or channel: an attention readout after the --readout statistics, gated per row or per element")
    p.add_argument("--pool", type=str, default="none",
                   help="none, topk or sag: a pooling layer (ops.TopKPooling / ops.SAGPooling) after every conv layer but the last; "
                        "the readout is taken on the last level")
    p.add_argument("--pool_ratio", type=float, default=0.5, help="the share of its nodes every graph keeps at a pooling layer")
    p.add_argument("--fused_pool", type=_bool, default=True, help="False: the pooling composed from torch ops")
    p.add_argument("--fused_readout", type=_bool, default=True, help="False: the readout composed from torch ops")
    p.add_argument("--norm", type=str, default="none",
                   help="none or graph: a per-graph normalisation (ops.GraphNorm) between every conv layer and its ReLU")
    p.add_argument("--fused_norm", type=_bool, default=True, help="False: the normalisation composed from torch ops")
    p.add_argument("--dim", type=int, default=32, help="input feature width")
    p.add_argument("--hidden", type=int, default=64, help="hidden width")
    p.add_argument("--classes", type=int, default=4, help="graph classes")
    p.add_argument("--num_layers", type=int, default=2, help="conv layers (>= 2)")
    p.add_argument("--num_epoches", type=int, default=20, help="epochs (passes over the collection)")
    p.add_argument("--partSize", type=int, default=32, help="neighbor-group size")
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--dtype", type=str, default="float32")
    p.add_argument("--verbose_mode", type=_bool, default=False)
    return p


def _parse(args):
    if args.model not in ("gcn", "gin", "gine", "schnet"):
        raise SystemExit("--model %s: graph_main trains gcn or gin (the other layers take a GraphBatch too: build the model with ops), "
                         "or gine with --edge_dim K" % args.model)
    if args.model == "gine" and args.edge_dim < 1:
        raise SystemExit("--model gine needs --edge_dim K with K >= 1: the features per edge (got %d)" % args.edge_dim)
    if args.model == "schnet":
        if args.cutoff is None or not 0.0 < args.cutoff < float("inf"):
            raise SystemExit("--model schnet needs --cutoff R with 0 < R < inf: the radius of the graph (got %r)" % args.cutoff)
        if args.max_neighbors is not None and not 1 <= args.max_neighbors <= 64:
            raise SystemExit("--max_neighbors must be in [1, 64] (got %d)" % args.max_neighbors)
        if args.num_gaussians < 2:
            raise SystemExit("--num_gaussians must be >= 2 (got %d)" % args.num_gaussians)
        if args.pool != "none" or args.norm != "none":
            raise SystemExit("--model schnet runs without --pool and --norm: a coarsened batch would need its graph rebuilt from the kept positions")
    elif args.cutoff is not None or args.max_neighbors is not None:
        raise SystemExit("--cutoff / --max_neighbors: only --model schnet builds its graph from positions (got --model %s)" % args.model)
    if args.model != "gine" and args.edge_dim != 0:
        raise SystemExit("--edge_dim %d: only --model gine takes edge features (got --model %s)" % (args.edge_dim, args.model))
    if args.dtype != "float32":
        raise SystemExit("--dtype %s: the readout (sum / mean / max / min over the rows of a graph) is float32 only; "
                         "run graph_main with --dtype float32" % args.dtype)
    try:
        lo, hi = (int(v) for v in args.graph_nodes.split(","))
    except ValueError:
        raise SystemExit("--graph_nodes takes MIN,MAX, e.g. 8,72 (got %r)" % args.graph_nodes)
    if lo < 1 or hi < lo:
        raise SystemExit("--graph_nodes needs 1 <= MIN <= MAX (got %r)" % args.graph_nodes)
    modes = tuple(m for m in args.readout.split(",") if m)
    from .ops import POOL_MODES
    if not modes or [m for m in modes if m not in POOL_MODES] or len(set(modes)) != len(modes):
        raise SystemExit("--readout takes a comma list of sum, mean, max, min, each once (got %r)" % args.readout)
    if args.attention_readout not in ("none", "scalar", "channel"):
        raise SystemExit("--attention_readout takes none, scalar or channel (got %r)" % args.attention_readout)
    if args.pool not in ("none", "topk", "sag"):
        raise SystemExit("--pool takes none, topk or sag (got %r)" % args.pool)
    if args.norm not in ("none", "graph"):
        raise SystemExit("--norm takes none or graph (got %r)" % args.norm)
    if not 0.0 < args.pool_ratio <= 1.0:
        raise SystemExit("--pool_ratio must be in (0, 1] (got %r)" % args.pool_ratio)
    if args.num_graphs < 1:
        raise SystemExit("--num_graphs must be >= 1")
    if args.batch_graphs < 1:
        raise SystemExit("--batch_graphs must be >= 1")
    if args.num_layers < 2:
        raise SystemExit("--num_layers must be >= 2 (got %d)" % args.num_layers)
    if args.num_epoches < 1:
        raise SystemExit("--num_epoches must be >= 1")
    return lo, hi, modes


def build_model(args, modes):
    from torch.nn import Linear, Module, ModuleList, ReLU, Sequential

    from .ops import AttentionalReadout, GCNConv, GINConv, GraphNorm, Readout, SAGPooling, TopKPooling
    if args.model == "schnet":
        from .spatial import SchNetInteraction

        class SchNet(Module):
            def __init__(self):
                super().__init__()
                self.embed = Linear(args.dim, args.hidden)
                self.layers = ModuleList(SchNetInteraction(args.hidden, args.hidden, args.num_gaussians, args.cutoff, fused=args.fused_edge)
                                         for _ in range(args.num_layers))
                self.readout = Readout(modes, fused=args.fused_readout)
                self.attention = AttentionalReadout(Linear(args.hidden, 1 if args.attention_readout == "scalar" else args.hidden),
                                                    fused=args.fused_readout) if args.attention_readout != "none" else None
                self.lin = Linear(args.hidden * (len(modes) + (1 if self.attention is not None else 0)), args.classes)

            def forward(self, x, batch):
                x = self.embed(x)
                for layer in self.layers:
                    x = layer(x, batch)
                pooled = self.readout(x, batch)
                if self.attention is not None:
                    pooled = torch.cat((pooled, self.attention(x, batch)), 1)
                return torch.log_softmax(self.lin(pooled), dim=1)

        return SchNet()
    conv = GCNConv if args.model == "gcn" else GINConv
    gine = args.model == "gine"
    if gine:
        from .edgeconv import GINEConv

        def edge_conv(a, b):
            return GINEConv(Sequential(Linear(a, b), ReLU(), Linear(b, b)), edge_dim=args.edge_dim, fused=args.fused_edge)
    attention = args.attention_readout != "none"

    class Net(Module):
        def __init__(self):
            super().__init__()
            dims = [args.dim] + [args.hidden] * args.num_layers
            self.convs = ModuleList((edge_conv if gine else conv)(a, b) for a, b in zip(dims[:-1], dims[1:]))
            # per-graph normalisation between every conv layer and its ReLU (its parameters start as constants: no random number)
            self.norms = ModuleList(GraphNorm(args.hidden, fused=args.fused_norm) for _ in self.convs) if args.norm == "graph" else None
            self.readout = Readout(modes, fused=args.fused_readout)
            # the learned readout next to the statistics: its gate scores every row (scalar) or every element (channel)
            self.attention = AttentionalReadout(Linear(args.hidden, 1 if args.attention_readout == "scalar" else args.hidden),
                                                fused=args.fused_readout) if attention else None
            self.lin = Linear(args.hidden * (len(modes) + (1 if attention else 0)), args.classes)
            # hierarchical pooling: every conv layer but the last hands a coarsened batch to the next one
            self.pools = None
            if args.pool != "none":
                pool = (lambda: TopKPooling(args.hidden, ratio=args.pool_ratio, fused=args.fused_pool)) if args.pool == "topk" else \
                    (lambda: SAGPooling(args.hidden, ratio=args.pool_ratio, GNN=conv, fused=args.fused_pool))
                self.pools = ModuleList(pool() for _ in range(args.num_layers - 1))
            self.levels = []           # (rows, edges) of every level of the latest forward pass

        def forward(self, x, batch):
            levels = [(batch.num_nodes, int(batch.column_index.numel()))]
            for k, layer in enumerate(self.convs):
                x = layer(x, batch, batch.edge_attr) if gine else layer(x, batch)
                if self.norms is not None:
                    x = self.norms[k](x, batch)
                x = torch.relu(x)
                if self.pools is not None and k < len(self.pools):
                    x, batch, _selection, _gate = self.pools[k](x, batch)
                    levels.append((batch.num_nodes, int(batch.column_index.numel())))
            self.levels = levels
            pooled = self.readout(x, batch)
            if self.attention is not None:
                pooled = torch.cat((pooled, self.attention(x, batch)), 1)
            return torch.log_softmax(self.lin(pooled), dim=1)

    return Net()


def make_dataset(args, lo, hi, device):
    from .batching import GraphDataset
    from .graph import small_graphs
    rp, ci, gp = small_graphs(args.num_graphs, lo, hi, args.avg_degree, seed=args.seed, device=device)
    g = torch.Generator()
    g.manual_seed(args.seed + 1)
    n = int(rp.numel()) - 1
    x = torch.randn(n, args.dim, generator=g)
    sizes = (gp[1:] - gp[:-1]).cpu().long()
    which = torch.repeat_interleave(torch.arange(args.num_graphs), sizes)
    mean0 = torch.zeros(args.num_graphs).index_add_(0, which, x[:, 0]) / sizes.clamp(min=1).float()
    # classes by the quantiles of (size, mean of feature 0): something a sum or mean readout can learn
    score = (sizes.float() - sizes.float().mean()) / (sizes.float().std() + 1e-6) + 4.0 * mean0
    order = score.argsort()
    y = torch.empty(args.num_graphs, dtype=torch.int64)
    y[order] = torch.arange(args.num_graphs) * args.classes // args.num_graphs
    if args.model != "gine":
        return GraphDataset(rp, ci, gp, x.to(device), y.to(device))
    # one row of K features per edge, each direction of an undirected edge on its own (e_ij != e_ji); the label moves with the mean
    # of their first column, which only a layer that reads the edge features can see
    rp_h = rp.cpu().long()
    nnz = int(rp_h[-1])
    edge_attr = torch.randn(nnz, args.edge_dim, generator=g)
    edge_graph = which[torch.repeat_interleave(torch.arange(n), rp_h[1:] - rp_h[:-1])]
    edges = torch.zeros(args.num_graphs).index_add_(0, edge_graph, torch.ones(nnz))
    emean0 = torch.zeros(args.num_graphs).index_add_(0, edge_graph, edge_attr[:, 0]) / edges.clamp(min=1)
    order = (score + 4.0 * emean0).argsort()
    y[order] = torch.arange(args.num_graphs) * args.classes // args.num_graphs
    return GraphDataset(rp, ci, gp, x.to(device), y.to(device), edge_attr=edge_attr.to(device))


class PointBatch(object):
    """The graphs [first, last) of a point-set collection: positions, pointers, features and labels; its graph is built per step."""

    def __init__(self, pos, gp, x, y, first, last):
        lo, hi = int(gp[first]), int(gp[last])
        self.pos, self.x, self.y = pos[lo:hi], x[lo:hi], y[first:last]
        self.graph_pointers = (gp[first:last + 1] - lo).to(torch.int32).to(pos.device)
        self.num_graphs = last - first


def make_point_batches(args, lo, hi, device, B):
    """(the PointBatch list of --model schnet, nodes in all): graph.small_point_clouds, node features as make_dataset draws them."""
    from .graph import small_point_clouds
    pos, gp, y = small_point_clouds(args.num_graphs, lo, hi, dim=3, density=args.density, seed=args.seed, classes=args.classes)
    g = torch.Generator()
    g.manual_seed(args.seed + 1)
    x = torch.randn(int(gp[-1]), args.dim, generator=g)
    pos, x, y = pos.to(device), x.to(device), y.to(device)
    return [PointBatch(pos, gp, x, y, k, min(k + B, args.num_graphs)) for k in range(0, args.num_graphs, B)], int(gp[-1])


def main(argv=None, capture=None):
    args = build_parser().parse_args(argv)
    lo, hi, modes = _parse(args)
    if not torch.cuda.is_available():
        raise SystemExit("graph_main needs a GPU: there is no CPU path in libgnna")
    device = torch.device("cuda")
    torch.manual_seed(args.seed)
    schnet = args.model == "schnet"
    B = min(args.batch_graphs, args.num_graphs)
    if schnet:
        return train_schnet(args, lo, hi, modes, device, B, capture)
    dataset = make_dataset(args, lo, hi, device)
    model = build_model(args, modes).to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr)
    # the mini-batches are the same every epoch: cut them out once (each is a few arrays on the device)
    ids = torch.arange(args.num_graphs, device=device)
    # (gine: a directed batch finds an edge's features in the backward through the perm of its device-built transpose; the
    # reverse-edge map of a symmetric one is made on the host)
    kw = {"directed": True} if args.model == "gine" else {}
    batches = [dataset.batch(ids[k: k + B], partSize=args.partSize, hiddenDim=args.hidden, **kw) for k in range(0, args.num_graphs, B)]
    if args.verbose_mode:
        print("# %d graphs, %d nodes, %d edges, %d batches of up to %d graphs, readout %s (%s)" % (
            args.num_graphs, dataset.num_nodes, int(dataset.column_index.numel()), len(batches), B, ",".join(modes),
            "fused" if args.fused_readout else "composed"))
        if args.attention_readout != "none":
            print("# attention readout: one score per %s" % ("row" if args.attention_readout == "scalar" else "element"))
        if args.model == "gine":
            print("# edge features: %d per edge, GINEConv (%s)" % (args.edge_dim, "fused" if args.fused_edge else "composed"))
        if args.norm != "none":
            print("# normalisation: GraphNorm after every conv layer (%s)" % ("fused" if args.fused_norm else "composed"))

    def epoch():
        total = torch.zeros((), device=device)
        for b in batches:
            optimizer.zero_grad(set_to_none=True)
            loss = torch.nn.functional.nll_loss(model(b.x, b), b.y)
            loss.backward()
            optimizer.step()
            total += loss.detach() * b.num_graphs
        return total / args.num_graphs

    model.train()
    first = epoch()                                   # dry run; also the loss after one epoch
    if capture is not None:
        capture.update(first_loss=float(first))
    if args.verbose_mode:
        print("# loss after 1 epoch: {:.6f}".format(float(first)))
        if args.pool != "none":
            print("# pooling %s at ratio %g (%s); the last batch, level by level: %s" % (
                args.pool, args.pool_ratio, "fused" if args.fused_pool else "composed",
                ", ".join("%d rows %d edges" % level for level in model.levels)))
    torch.cuda.synchronize()
    start = time.perf_counter()
    for _ in range(args.num_epoches):
        loss = epoch()
    torch.cuda.synchronize()
    train_time = time.perf_counter() - start
    if capture is not None:
        capture.update(final_loss=float(loss), epoch_ms=train_time * 1e3 / args.num_epoches)
    if args.verbose_mode:
        print("# final loss: {:.6f}".format(float(loss)))
    print('Time (ms): {:.3f}'.format(train_time * 1e3 / args.num_epoches))
    print()
    return 0


def train_schnet(args, lo, hi, modes, device, B, capture):
    """--model schnet: every step builds its mini-batch's graph on the device from the batch's positions."""
    from . import spatial
    batches, nodes = make_point_batches(args, lo, hi, device, B)
    model = build_model(args, modes).to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr)
    seen = {"edges": 0, "graph_ms": 0.0}

    def graph_of(b):
        batch = spatial.radius_graph(b.pos, args.cutoff, b.graph_pointers, max_num_neighbors=args.max_neighbors, partSize=args.partSize,
                                     fused=args.fused_graph, hiddenDim=args.hidden)
        seen["edges"] += int(batch.column_index.numel())
        return batch

    def epoch(timed=False):
        total = torch.zeros((), device=device)
        seen["edges"] = 0
        for b in batches:
            if timed:
                torch.cuda.synchronize()
                start = time.perf_counter()
            batch = graph_of(b)
            if timed:
                torch.cuda.synchronize()
                seen["graph_ms"] += (time.perf_counter() - start) * 1e3
            optimizer.zero_grad(set_to_none=True)
            loss = torch.nn.functional.nll_loss(model(b.x, batch), b.y)
            loss.backward()
            optimizer.step()
            total += loss.detach() * b.num_graphs
        return total / args.num_graphs

    model.train()
    first = epoch()                                   # dry run; also the loss after one epoch
    if capture is not None:
        capture.update(first_loss=float(first), num_edges=seen["edges"], num_nodes=nodes)
    if args.verbose_mode:
        print("# %d point sets, %d nodes, %d batches of up to %d graphs, readout %s (%s)" % (
            args.num_graphs, nodes, len(batches), B, ",".join(modes), "fused" if args.fused_readout else "composed"))
        print("# radius graph: cutoff %g, %s, built per step (%s): %d nodes %d edges per epoch" % (
            args.cutoff, "no cap" if args.max_neighbors is None else "at most %d neighbours" % args.max_neighbors,
            "fused" if args.fused_graph else "composed", nodes, seen["edges"]))
        print("# loss after 1 epoch: {:.6f}".format(float(first)))
    torch.cuda.synchronize()
    start = time.perf_counter()
    for _ in range(args.num_epoches):
        loss = epoch()
    torch.cuda.synchronize()
    train_time = time.perf_counter() - start
    if capture is not None:
        capture.update(final_loss=float(loss), epoch_ms=train_time * 1e3 / args.num_epoches)
    if args.verbose_mode:
        epoch(timed=True)                             # one more epoch with a synchronisation around every graph build
        print("# graph construction: {:.3f} ms of an epoch (synchronised around every build)".format(seen["graph_ms"]))
        if capture is not None:
            capture.update(graph_ms=seen["graph_ms"])
        print("# final loss: {:.6f}".format(float(loss)))
    print('Time (ms): {:.3f}'.format(train_time * 1e3 / args.num_epoches))
    print()
    return 0


if __name__ == '__main__':
    sys.exit(main())
