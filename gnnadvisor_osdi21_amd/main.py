#!/usr/bin/env python3
"""Training / profiling driver: ``python -m gnnadvisor_osdi21_amd.main [flags]``.

Counterpart of the reference's GNNAdvisor/GNNA_main.py: the same command-line flags
(:15-39, booleans are the strings 'True'/'False'), the same stages (load -> inputProperty ->
decider -> build_part -> verify | single-SpMM profile | train, :59-202), the same models
(2-layer GCN :143-153, 5-layer GIN :155-171), optimiser (Adam lr=0.01 :178), loss
(nll_loss of log_softmax vs all-ones labels :185) and the same printed lines that the
reference's log scrapers key on (``print(args)`` with ``dataset='x',`` and
``Time (ms): %.3f``, 1_log2csv.py:13-20).  Extra flags: ``--synthetic NAME`` (seeded stand-in
graph instead of a file, since no dataset ships) and ``--policy`` (Decider policy).
"""
import argparse
import os.path as osp
import sys
import time

import torch
import torch.nn.functional as F


class _Parser(argparse.ArgumentParser):
    """argparse takes `--fanout -1,-1` for two options: the value is joined to its flag before parsing."""

    def parse_known_args(self, args=None, namespace=None):
        args = list(sys.argv[1:] if args is None else args)
        for i in range(len(args) - 2, -1, -1):
            if args[i] == "--fanout":
                args[i: i + 2] = ["--fanout=" + args[i + 1]]
        return super().parse_known_args(args, namespace)


def build_parser():
    p = _Parser()
    p.add_argument("--dataDir", type=str, default="../osdi-ae-graphs", help="the path to graphs")
    p.add_argument("--dataset", type=str, default='amazon0601', help="dataset")
    p.add_argument("--dim", type=int, default=96, help="input embedding dimension size")
    p.add_argument("--hidden", type=int, default=16, help="hidden dimension size")
    p.add_argument("--classes", type=int, default=22, help="output classes size")
    p.add_argument('--model', type=str, default='gcn', choices=['gcn', 'gin', 'gat', 'gatv2', 'transformer', 'sage', 'rgcn', 'pna', 'gen'],
                   help="GCN, GIN, GAT, GATv2 (dynamic attention, two layers as gat), graph transformer (dot-product attention, two "
                        "TransformerConv layers as gat), GraphSAGE, R-GCN, PNA (two PNAConv layers: mean, max, min and std from one gather) "
                        "or GEN (two GENConv layers: softmax aggregation with a temperature from one gather)")
    p.add_argument('--softmax_t', type=float, default=1.0, help="--model gen: the (initial) temperature of the softmax aggregation")
    p.add_argument('--learn_t', default='False', choices=['True', 'False'],
                   help="--model gen: True learns the temperature of each layer (one value per layer)")
    p.add_argument('--num_relations', type=int, default=4,
                   help="--model rgcn: relation types of the edges (synthetic: a seeded hash of every edge's end points)")
    p.add_argument('--num_bases', type=int, default=0,
                   help="--model rgcn: bases of the weight decomposition W_r = sum_b c[r, b] V_b (0: none, one weight per relation)")
    p.add_argument('--aggregator', type=str, default='mean', choices=['mean', 'max', 'min'],
                   help="GraphSAGE: how a node's neighbours are reduced (mean, element-wise max or element-wise min)")
    p.add_argument('--heads', type=int, default=1, help="GAT, GATv2, transformer: attention heads of the hidden layer (the output layer has one)")
    p.add_argument("--num_epoches", type=int, default=200, help="number of epoches for training, default=200")
    p.add_argument("--partSize", type=int, default=32, help="neighbor-group size")
    p.add_argument("--dimWorker", type=int, default=32, help="number of worker threads (hint on MI355X)")
    p.add_argument("--warpPerBlock", type=int, default=4, help="wavefronts per block (hint on MI355X)")
    p.add_argument("--sharedMem", type=int, default=100, help="shared memory (KB) assumed by the compat Decider policy")
    tf = dict(type=str, choices=['True', 'False'])
    p.add_argument('--manual_mode', default='True', help="True: manual config, False: auto config", **tf)
    p.add_argument('--verbose_mode', default='False', help="True: verbose mode", **tf)
    p.add_argument('--enable_rabbit', default='False', help="True: enable locality reordering", **tf)
    p.add_argument('--loadFromTxt', default='False', help="True: load a TXT edge list, False: .npz", **tf)
    p.add_argument('--single_spmm', default='False', help="True: profile one SpMM for num_epoches rounds", **tf)
    p.add_argument('--verify_spmm', default='False', help="True: verify one SpMM against the CPU reference", **tf)
    p.add_argument('--synthetic', type=str, default=None, help="use a seeded synthetic graph (graph.CONFIGS name)")
    p.add_argument('--scale', type=float, default=1.0, help="shrink the synthetic graph")
    p.add_argument('--locality', type=float, default=0.0, help="synthetic graph: share of the edges within +-4096 ids of a hidden order")
    p.add_argument('--scramble', default='False', **tf, help="synthetic graph: relabel the nodes at random (hides the locality)")
    p.add_argument('--dtype', type=str, default='float32', choices=['float32', 'bfloat16', 'float16'],
                   help="element type of the features and the model (gcn, gin): bfloat16 / float16 are aggregated with fp32 "
                        "accumulation (libgnna gnna_agg_ld_x16); float16 GCN outputs can overflow on hub rows, prefer bfloat16")
    p.add_argument('--hip_graph', default='False', **tf,
                   help="True: capture one training epoch (forward, backward, Adam) into a HIP graph and replay it "
                        "(MI355X addition; pays on small, launch-bound graphs)")
    p.add_argument('--tune_gemm', default='False', **tf,
                   help="True: let PyTorch's TunableOp time the rocBLAS / hipBLASLt solutions for the layer GEMMs at "
                        "first use (X W and G W^T run 1.3-2x faster; costs 1-2 minutes of set-up, MI355X addition)")
    p.add_argument('--fused_attention', default='False', **tf,
                   help="True: --model gat runs both layers on the fused attention kernels (GATConv(fused=True): alpha is made "
                        "from node-sized values where the rows are gathered, no per-edge tensor; MI355X addition); --model gatv2 likewise "
                        "(GATv2Conv(fused=...): False is the composed path with [nnz, heads * hidden] tensors) and --model transformer "
                        "(TransformerConv(fused=...))")
    p.add_argument('--attn_drop', type=float, default=0.0,
                   help="--model gat: dropout on the attention coefficients of both layers while training (GATConv(attn_drop=P), "
                        "P in [0, 1); 0.6 in the GAT paper).  With --fused_attention True the mask is made inside the kernels from "
                        "one host-drawn seed per layer and step, with --fanout too; a captured HIP graph would replay one seed and "
                        "so one mask, one more reason --hip_graph stays refused for --model gat (MI355X addition); --model gatv2 and --model transformer likewise")
    p.add_argument('--edge_dim', type=int, default=0,
                   help="--model gat: D > 0 gives both layers edge features in the score (GATConv(edge_dim=D): one scalar per edge "
                        "and head before the leaky ReLU, as PyG's GATConv(edge_dim=...)).  The driver draws synthetic features "
                        "[nnz, D] from a seeded generator once the graph's CSR is fixed; with --fanout every block takes the rows of "
                        "its own edges (SampledBlock.edge_ids).  0: none (MI355X addition)")
    p.add_argument('--directed', default='False', **tf,
                   help="True: the graph is directed -- every backward pass aggregates over the transposed structure, built on "
                        "the device right after the partition (False: the structure is taken to be symmetric, as the "
                        "reference does, and the backward passes reuse the forward graph)")
    p.add_argument('--fanout', type=str, default=None,
                   help="--model sage / pna / gen, or --model gat / gatv2 / transformer with --fused_attention True: train on sampled mini-batches -- a comma list "
                        "with one entry per layer, the neighbours sampled per node at that layer (-1: all of them), e.g. 25,10; "
                        "the blocks are drawn on the device (sampling.NeighborSampler, MI355X addition)")
    p.add_argument('--batch_size', type=int, default=1024, help="--fanout: seed nodes per mini-batch")
    p.add_argument('--saint_roots', type=int, default=None,
                   help="with --walk_length: train on GraphSAINT random-walk subgraphs -- every step walks --walk_length steps from "
                        "this many random roots on the device and trains on the subgraph the visited nodes induce, at full depth "
                        "(sampling.SaintRWSampler, MI355X addition); every model whose layers take a graph batch (all but rgcn)")
    p.add_argument('--walk_length', type=int, default=None, help="--saint_roots: steps of every walk (GraphSAINT-RW on Reddit: 2)")
    p.add_argument('--saint_steps', type=int, default=8, help="--saint_roots: subgraphs (optimiser steps) per epoch")
    p.add_argument('--saint_coverage', type=int, default=0,
                   help="--saint_roots: T > 0 pre-samples T subgraphs and weighs every node's loss by GraphSAINT's T / (N C_v) "
                        "(SaintRWSampler.estimate_norms); 0: the plain mean over the subgraph's nodes")
    p.add_argument('--policy', type=str, default='mi355x', choices=['mi355x', 'compat'], help="Decider policy")
    p.add_argument('--force_rabbit', default='False', **tf,
                   help="True: with --enable_rabbit True in auto mode, renumber even when the mi355x cost gate says the run is "
                        "too short to win the host seconds back (MI355X addition)")
    return p


def main(argv=None, capture=None):
    """capture: a dict that receives the run's objects (dataset, inputInfo, model) -- for tests and notebooks."""
    args = build_parser().parse_args(argv)
    print(args)
    flag = lambda s: s == 'True'
    partSize, dimWorker, warpPerBlock, sharedMem = args.partSize, args.dimWorker, args.warpPerBlock, args.sharedMem
    manual_mode, verbose_mode = flag(args.manual_mode), flag(args.verbose_mode)
    enable_rabbit, loadFromTxt = flag(args.enable_rabbit), flag(args.loadFromTxt)
    single_spmm, verify_spmm = flag(args.single_spmm), flag(args.verify_spmm)

    attention = args.model in ('gat', 'gatv2', 'transformer')      # the attention models share their flags and refusals
    if attention and flag(args.hip_graph):
        # (the attention layers build their per-edge arrays and the SDDMM's id copies at first use: not captured yet)
        raise SystemExit("--model %s does not support --hip_graph True: run it with --hip_graph False" % args.model)
    if args.dtype != 'float32' and attention:
        raise SystemExit("--dtype %s: the attention layers (edge-weighted aggregation, SDDMM, edge softmax) are float32 only; "
                         "run --model %s with --dtype float32" % (args.dtype, args.model))
    if args.dtype != 'float32' and args.model == 'sage':
        raise SystemExit("--dtype %s: the GraphSAGE layers (max / min / mean over the neighbours) are float32 only; "
                         "run --model sage with --dtype float32" % args.dtype)
    if args.dtype != 'float32' and args.model == 'pna':
        raise SystemExit("--dtype %s: the PNA layers (mean / std / max / min over the neighbours from one gather) are float32 only; "
                         "run --model pna with --dtype float32" % args.dtype)
    if args.dtype != 'float32' and args.model == 'gen':
        raise SystemExit("--dtype %s: the GEN layers (softmax aggregation over the neighbours from one gather) are float32 only; "
                         "run --model gen with --dtype float32" % args.dtype)
    if args.model == 'rgcn':
        if flag(args.hip_graph):
            # (the relational graph builds its transposed structure and permuted edge arrays at the first backward: not captured)
            raise SystemExit("--model rgcn does not support --hip_graph True: run it with --hip_graph False")
        if args.dtype != 'float32':
            raise SystemExit("--dtype %s: the R-GCN layers (relation-typed aggregation) are float32 only; "
                             "run --model rgcn with --dtype float32" % args.dtype)
        if args.num_relations < 1:
            raise SystemExit("--num_relations must be >= 1")
        if not 0 <= args.num_bases <= 16:
            raise SystemExit("--num_bases must be in 0 .. 16 (0: no decomposition)")
        if args.num_bases == 0 and args.num_relations > 16:
            raise SystemExit("--model rgcn without bases supports at most 16 relations: pass --num_bases")
    if args.dtype != 'float32' and flag(args.hip_graph):
        raise SystemExit("--dtype %s does not support --hip_graph True yet: run it with --hip_graph False" % args.dtype)
    if args.dtype != 'float32' and (flag(args.single_spmm) or flag(args.verify_spmm)):
        raise SystemExit("--single_spmm / --verify_spmm run the float32 entry: use --dtype float32")
    if args.heads < 1:
        raise SystemExit("--heads must be >= 1")
    if flag(args.fused_attention) and not attention:
        raise SystemExit("--fused_attention True selects the fused GAT attention: run it with --model gat (got --model %s)" % args.model)
    if args.attn_drop != 0.0 and not attention:
        raise SystemExit("--attn_drop drops attention coefficients: run it with --model gat (got --model %s)" % args.model)
    if not 0.0 <= args.attn_drop < 1.0:
        raise SystemExit("--attn_drop must be in [0, 1) (got %r)" % args.attn_drop)
    if args.edge_dim < 0:
        raise SystemExit("--edge_dim must be >= 0 (got %d)" % args.edge_dim)
    if args.edge_dim > 0 and args.model != 'gat':
        raise SystemExit("--edge_dim puts edge features into the GAT score: run it with --model gat (got --model %s)" % args.model)
    fanouts = None
    if args.fanout is not None:
        if attention and not flag(args.fused_attention):
            raise SystemExit("--model %s --fanout runs on the fused attention kernels only (the composed path would build "
                             "per-edge tensors for every batch): add --fused_attention True" % args.model)
        if args.model not in ('sage', 'pna', 'gen', 'gat', 'gatv2', 'transformer'):
            raise SystemExit("--fanout trains GraphSAGE on sampled blocks: run it with --model sage, or with --model gat "
                             "--fused_attention True (got --model %s)" % args.model)
        if flag(args.hip_graph):
            raise SystemExit("--fanout does not support --hip_graph True: every batch samples new blocks and reads their sizes "
                             "back; run it with --hip_graph False")
        if args.dtype != 'float32':
            raise SystemExit("--fanout: the layers that take a block are float32 only; use --dtype float32")
        if single_spmm or verify_spmm:
            raise SystemExit("--fanout does not go with --single_spmm / --verify_spmm: they run one full-graph aggregation")
        try:
            fanouts = [int(f) for f in args.fanout.split(",")]
        except ValueError:
            raise SystemExit("--fanout takes a comma list of integers, e.g. 25,10 (got %r)" % args.fanout)
        if len(fanouts) != 2:
            raise SystemExit("--fanout needs one entry per layer: --model %s has 2 layers (got %d)" % (args.model, len(fanouts)))
        if args.batch_size < 1:
            raise SystemExit("--batch_size must be >= 1")
    saint = args.saint_roots is not None or args.walk_length is not None
    if saint:
        if args.saint_roots is None or args.walk_length is None:
            raise SystemExit("--saint_roots and --walk_length come together: the roots per step and the steps of every walk")
        if fanouts is not None:
            raise SystemExit("--saint_roots does not go with --fanout: one trains on induced subgraphs at full depth, the other "
                             "on per-layer blocks; pass one of them")
        if args.model == 'rgcn':
            raise SystemExit("--saint_roots trains on induced subgraphs, which --model rgcn does not take (its layers run on a "
                             "relational.RelationalGraph): run it with one of gcn, gin, sage, gat, gatv2, transformer, pna, gen")
        if flag(args.hip_graph):
            raise SystemExit("--saint_roots does not support --hip_graph True: every step cuts a new subgraph and reads its sizes "
                             "back; run it with --hip_graph False")
        if args.dtype != 'float32':
            raise SystemExit("--saint_roots: the subgraph steps are float32 only; use --dtype float32")
        if single_spmm or verify_spmm:
            raise SystemExit("--saint_roots does not go with --single_spmm / --verify_spmm: they run one full-graph aggregation")
        if args.saint_roots < 1:
            raise SystemExit("--saint_roots must be >= 1")
        if args.walk_length < 0:
            raise SystemExit("--walk_length must be >= 0")
        if args.saint_steps < 1:
            raise SystemExit("--saint_steps must be >= 1")
        if args.saint_coverage < 0:
            raise SystemExit("--saint_coverage must be >= 0")
    elif args.saint_steps != 8 or args.saint_coverage != 0:
        raise SystemExit("--saint_steps and --saint_coverage belong to --saint_roots: pass --saint_roots R --walk_length L")
    assert torch.cuda.is_available(), "requires an MI355X GPU: there is no CPU path"
    device = torch.device('cuda')
    if flag(args.tune_gemm):
        import tempfile
        import torch.cuda.tunable as tunable
        tunable.enable(True)
        tunable.tuning_enable(True)
        tunable.set_max_tuning_duration(50)
        tunable.set_max_tuning_iterations(10)
        tunable.set_filename(osp.join(tempfile.gettempdir(), "gnna_tunableop.csv"))   # keep the results out of the cwd

    from . import load_extension
    from .decider import inputProperty
    from .loader import custom_dataset
    from .ops import GATConv, GATv2Conv, GCNConv, GENConv, GINConv, PNAConv, RGCNConv, SAGEConv, TransformerConv
    from .structure import backward_structure
    GNNA = load_extension()

    # ---- loading data --------------------------------------------------------------------
    if args.synthetic:
        dataset = custom_dataset.from_synthetic(args.synthetic, args.dim, args.classes, args.scale,
                                                verbose=verbose_mode, device=device, locality=args.locality,
                                                scramble=flag(args.scramble))
    elif loadFromTxt:
        dataset = custom_dataset(osp.join(args.dataDir, args.dataset), args.dim, args.classes,
                                 load_from_txt=True, verbose=verbose_mode, device=device)
    else:
        dataset = custom_dataset(osp.join(args.dataDir, args.dataset + ".npz"), args.dim, args.classes,
                                 load_from_txt=False, verbose=verbose_mode, device=device)

    # ---- input property profile + Decider ---------------------------------------------------
    inputInfo = inputProperty(dataset.row_pointers, dataset.column_index, dataset.degrees,
                              partSize, dimWorker, warpPerBlock, sharedMem,
                              hiddenDim=args.hidden, dataset_obj=dataset, enable_rabbit=enable_rabbit,
                              manual_mode=manual_mode, verbose=verbose_mode, policy=args.policy)
    # what the run ahead will aggregate (the mi355x renumbering gate weighs the host seconds of a renumbering against it)
    from .decider import expected_aggregations
    inputInfo.expected_aggregations = [(args.hidden, args.num_epoches)] if (single_spmm or verify_spmm) else \
        expected_aggregations('gat' if args.model in ('gatv2', 'transformer') else args.model, dataset.num_features, args.hidden, dataset.num_classes, args.num_epoches + 10,
                              heads=args.heads, aggregator=args.aggregator, num_relations=args.num_relations,
                              num_bases=args.num_bases)
    inputInfo.force_renumbering = flag(args.force_rabbit)
    inputInfo.decider()
    inputInfo = inputInfo.set_input()
    if verbose_mode:
        print('----------------------------')
        inputInfo.print_param()
        print()
    inputInfo = inputInfo.set_hidden()
    if verbose_mode:
        inputInfo.print_param()
        print()
        print('----------------------------')

    # ---- neighbor partitioning -----------------------------------------------------------------
    start = time.perf_counter()
    partPtr, part2Node = GNNA.build_part(inputInfo.partSize, inputInfo.row_pointers)
    if verbose_mode:
        print("# Build nb_part (s): {:.3f}".format(time.perf_counter() - start))
    inputInfo.row_pointers = inputInfo.row_pointers.to(device)
    inputInfo.column_index = inputInfo.column_index.to(device)
    inputInfo.partPtr = partPtr.int().to(device)
    inputInfo.part2Node = part2Node.int().to(device)
    inputInfo.apply_tuning()      # scheduler knobs + this graph's hints (keyed by the device column_index)
    # graph lifecycle: the counting pass, its one synchronisation and the scratch sizing happen here, next to
    # build_part, instead of inside the first aggregation -- no epoch (and no captured epoch) synchronises or allocates
    from . import _lib as _gnna_lib
    _prep_widths = sorted({args.hidden, dataset.num_classes, dataset.num_features} |
                          ({2 * args.hidden} if args.model == 'pna' else set()))      # (PNA's backward sums [a | b] at 2 x hidden)
    _gnna_lib.prepare_graph(inputInfo.column_index, inputInfo.partPtr, inputInfo.part2Node, dataset.num_nodes,
                            dataset.num_nodes, inputInfo.partSize, _prep_widths)
    if not manual_mode and not (verify_spmm or single_spmm):
        # measured schedule for the widths the layers aggregate at (hidden, classes; GIN layer 1 aggregates
        # at the input width unless it is evaluated update-first)
        widths = {args.hidden, dataset.num_classes}
        if args.model == 'gin' and dataset.num_features <= 2 * args.hidden:
            widths.add(dataset.num_features)
        inputInfo.calibrate(widths)
        # the measured schedule may use other phase counts than the rule's: make their packed id copies now, not in an epoch
        _gnna_lib.prepare_graph(inputInfo.column_index, inputInfo.partPtr, inputInfo.part2Node, dataset.num_nodes,
                                dataset.num_nodes, inputInfo.partSize, _prep_widths)
    inputInfo.directed = flag(args.directed)
    if inputInfo.directed:
        # the backward passes' structure: built (and prepared like the forward graph) here, never inside a captured epoch
        start = time.perf_counter()
        # (composed attention is edge-valued: its backward reads the weights through the position map, so that is built too)
        edge_valued = attention and not flag(args.fused_attention)
        t_graph = backward_structure(inputInfo, edge_pos=True)[0] if edge_valued else backward_structure(inputInfo)
        torch.cuda.synchronize()
        if verbose_mode:
            print("# Build transposed graph on the device (s): {:.3f}".format(time.perf_counter() - start))
        _gnna_lib.prepare_graph(t_graph.column_index, t_graph.partPtr, t_graph.part2Node, dataset.num_nodes,
                                dataset.num_nodes, inputInfo.partSize, _prep_widths)
        if not manual_mode and not (verify_spmm or single_spmm):
            # the measured schedule, for the transposed ids' own layout
            from .decider import calibrate_phases
            calibrate_phases(t_graph.column_index, t_graph.partPtr, t_graph.part2Node, dataset.num_nodes, inputInfo.partSize,
                             widths, verbose=verbose_mode)
            _gnna_lib.prepare_graph(t_graph.column_index, t_graph.partPtr, t_graph.part2Node, dataset.num_nodes,
                                    dataset.num_nodes, inputInfo.partSize, _prep_widths)
    degrees = inputInfo.degrees
    edge_attr = None
    if args.edge_dim > 0:
        # synthetic edge features in the order of the column_index the Decider has settled on (a renumbering is behind us)
        gen = torch.Generator(device='cpu').manual_seed(0xED6E)
        edge_attr = torch.randn(inputInfo.column_index.numel(), args.edge_dim, generator=gen).to(device)
        if inputInfo.directed or (flag(args.fused_attention) and args.fanout is None):
            # the source-side pass reads the edge term through the position map of the backward structure (the permutation, or
            # the reverse-edge map, which also settles the symmetry question): built here, not inside the first step
            backward_structure(inputInfo, edge_pos=True)
    if capture is not None:
        capture.update(dataset=dataset, inputInfo=inputInfo, args=args, edge_attr=edge_attr)

    # ---- single-SpMM verification / profiling (GNNA_main.py:116-137) -------------------------------
    if verify_spmm or single_spmm:
        from .verify import Verification
        # like the reference, the CLI knobs (not the Decider's) are passed here (GNNA_main.py:119-122)
        valid = Verification(args.hidden, inputInfo.row_pointers, inputInfo.column_index, degrees,
                             inputInfo.partPtr, inputInfo.part2Node,
                             inputInfo.partSize, dimWorker, warpPerBlock)
        if verify_spmm:
            valid.compute()
            valid.reference(dataset.edge_index, dataset.val, dataset.num_nodes)
            valid.compare()
        else:
            valid.profile_spmm(round=args.num_epoches)
        return 0

    # ---- model ------------------------------------------------------------------------------------
    if args.model == 'gcn':
        class Net(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.conv1 = GCNConv(dataset.num_features, args.hidden)
                self.conv2 = GCNConv(args.hidden, dataset.num_classes)

            def forward(self):
                x = self.conv1(dataset.x, inputInfo.set_input(), relu=True)   # F.relu(conv1(...)), fused (GNNA_main.py:151)
                x = self.conv2(x, inputInfo.set_hidden())
                return F.log_softmax(x.float(), dim=1)
    elif args.model == 'gat':
        fused = flag(args.fused_attention)

        edge_dim = args.edge_dim if args.edge_dim > 0 else None

        def edges_of(block):         # the edge features of a block's own edges, or of the whole graph
            if edge_attr is None:
                return None
            return edge_attr if block is None else edge_attr.index_select(0, block.edge_ids.long())

        class Net(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.conv1 = GATConv(dataset.num_features, args.hidden, heads=args.heads, concat=True, fused=fused,
                                     attn_drop=args.attn_drop, edge_dim=edge_dim)
                self.conv2 = GATConv(args.hidden * args.heads, dataset.num_classes, heads=1, fused=fused, attn_drop=args.attn_drop,
                                     edge_dim=edge_dim)

            def forward(self, x=None, blocks=None):
                if blocks is not None:      # a sampled mini-batch (--fused_attention True): x holds blocks[0]'s source rows
                    x = F.elu(self.conv1(x, blocks[0], edge_attr=edges_of(blocks[0])))
                    x = self.conv2(x, blocks[1], edge_attr=edges_of(blocks[1]))
                    return F.log_softmax(x, dim=1)
                x = F.elu(self.conv1(dataset.x, inputInfo.set_input(), edge_attr=edges_of(None)))
                x = self.conv2(x, inputInfo.set_hidden(), edge_attr=edges_of(None))
                return F.log_softmax(x, dim=1)
    elif args.model == 'gatv2':
        fused = flag(args.fused_attention)

        class Net(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.conv1 = GATv2Conv(dataset.num_features, args.hidden, heads=args.heads, concat=True, fused=fused,
                                       attn_drop=args.attn_drop)
                self.conv2 = GATv2Conv(args.hidden * args.heads, dataset.num_classes, heads=1, fused=fused, attn_drop=args.attn_drop)

            def forward(self, x=None, blocks=None):
                if blocks is not None:      # a sampled mini-batch (--fused_attention True): x holds blocks[0]'s source rows
                    x = F.elu(self.conv1(x, blocks[0]))
                    x = self.conv2(x, blocks[1])
                    return F.log_softmax(x, dim=1)
                x = F.elu(self.conv1(dataset.x, inputInfo.set_input()))
                x = self.conv2(x, inputInfo.set_hidden())
                return F.log_softmax(x, dim=1)
    elif args.model == 'transformer':
        fused = flag(args.fused_attention)

        class Net(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.conv1 = TransformerConv(dataset.num_features, args.hidden, heads=args.heads, concat=True, fused=fused,
                                             attn_drop=args.attn_drop)
                self.conv2 = TransformerConv(args.hidden * args.heads, dataset.num_classes, heads=1, fused=fused,
                                             attn_drop=args.attn_drop)

            def forward(self, x=None, blocks=None):
                if blocks is not None:      # a sampled mini-batch (--fused_attention True): x holds blocks[0]'s source rows
                    x = F.elu(self.conv1(x, blocks[0]))
                    x = self.conv2(x, blocks[1])
                    return F.log_softmax(x, dim=1)
                x = F.elu(self.conv1(dataset.x, inputInfo.set_input()))
                x = self.conv2(x, inputInfo.set_hidden())
                return F.log_softmax(x, dim=1)
    elif args.model == 'sage':
        inputInfo.inv_row_counts()      # (the mean's row factors: built here, not inside a captured epoch)

        class Net(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.conv1 = SAGEConv(dataset.num_features, args.hidden, aggregator=args.aggregator)
                self.conv2 = SAGEConv(args.hidden, dataset.num_classes, aggregator=args.aggregator)

            def forward(self, x=None, blocks=None):
                if blocks is not None:      # a sampled mini-batch: x holds the rows of blocks[0]'s source nodes
                    x = self.conv1(x, blocks[0], relu=True)
                    x = self.conv2(x, blocks[1])
                    return F.log_softmax(x, dim=1)
                x = self.conv1(dataset.x, inputInfo.set_input(), relu=True)
                x = self.conv2(x, inputInfo.set_hidden())
                return F.log_softmax(x, dim=1)
    elif args.model == 'pna':
        # the row factors and the full graph's delta (mini-batches use it too): built here, not inside a captured epoch
        delta = PNAConv.delta_of(inputInfo)

        class Net(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.conv1 = PNAConv(dataset.num_features, args.hidden, delta=delta)
                self.conv2 = PNAConv(args.hidden, dataset.num_classes, delta=delta)

            def forward(self, x=None, blocks=None):
                if blocks is not None:      # a sampled mini-batch: x holds the rows of blocks[0]'s source nodes
                    x = self.conv1(x, blocks[0], relu=True)
                    x = self.conv2(x, blocks[1])
                    return F.log_softmax(x, dim=1)
                x = self.conv1(dataset.x, inputInfo.set_input(), relu=True)
                x = self.conv2(x, inputInfo.set_hidden())
                return F.log_softmax(x, dim=1)
    elif args.model == 'gen':
        class Net(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.conv1 = GENConv(dataset.num_features, args.hidden, t=args.softmax_t, learn_t=flag(args.learn_t))
                self.conv2 = GENConv(args.hidden, dataset.num_classes, t=args.softmax_t, learn_t=flag(args.learn_t))

            def forward(self, x=None, blocks=None):
                if blocks is not None:      # a sampled mini-batch: x holds the rows of blocks[0]'s source nodes
                    x = self.conv1(x, blocks[0], relu=True)
                    x = self.conv2(x, blocks[1])
                    return F.log_softmax(x, dim=1)
                x = self.conv1(dataset.x, inputInfo.set_input(), relu=True)
                x = self.conv2(x, inputInfo.set_hidden())
                return F.log_softmax(x, dim=1)
    elif args.model == 'rgcn':
        # the types are made here, from the CSR the kernels run on: a renumbering (decider) cannot misalign them
        from .relational import RelationalGraph, synthetic_edge_types
        rel = RelationalGraph(inputInfo, synthetic_edge_types(inputInfo.row_pointers, inputInfo.column_index,
                                                              args.num_relations, seed=0x52474E), args.num_relations)
        rel.transposed()                # (the second layer's feature gradient runs on it: built here, not inside an epoch)
        bases = args.num_bases or None
        if capture is not None:
            capture.update(rel=rel)

        class Net(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.conv1 = RGCNConv(dataset.num_features, args.hidden, args.num_relations, num_bases=bases)
                self.conv2 = RGCNConv(args.hidden, dataset.num_classes, args.num_relations, num_bases=bases)

            def forward(self):
                x = self.conv1(dataset.x, rel, relu=True)
                x = self.conv2(x, rel)
                return F.log_softmax(x, dim=1)
    else:
        class Net(torch.nn.Module):
            def __init__(self):
                super().__init__()
                dims = [dataset.num_features] + [args.hidden] * 4 + [dataset.num_classes]
                self.convs = torch.nn.ModuleList(GINConv(a, b) for a, b in zip(dims[:-1], dims[1:]))

            def forward(self):
                x = dataset.x
                for i, conv in enumerate(self.convs):
                    # F.relu after every layer but the last (GNNA_main.py:166-169), fused where the aggregation ends the layer
                    x = conv(x, inputInfo.set_input() if i == 0 else inputInfo.set_hidden(), relu=i + 1 < len(self.convs))
                return F.log_softmax(x.float(), dim=1)

    model = Net().to(device)
    if args.dtype != 'float32':
        # features and parameters stored in 16 bits; every aggregation accumulates in fp32 and rounds its result once
        dataset.x = dataset.x.to(getattr(torch, args.dtype))
        model = model.to(getattr(torch, args.dtype))
        _gnna_lib.prepare_x16(dataset.num_nodes, dataset.num_nodes, _prep_widths, device=device)
    if capture is not None:
        capture.update(dataset=dataset, inputInfo=inputInfo, model=model, args=args)
    if verbose_mode:
        print(model)
    use_graph = flag(args.hip_graph)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01, capturable=use_graph)

    def nll_loss(log_prob, target):
        """F.nll_loss(log_prob, target) (mean over nodes, GNNA_main.py:186) written as gather + mean:
        torch's nll_loss reduces all N rows in ONE workgroup (0.5 ms forward + 0.3 ms backward at
        N = 410 K, 3.8 + 3.0 ms at N = 2.4 M -- a quarter of a GCN epoch); gather/mean are grid-wide."""
        return -log_prob.gather(1, target.view(-1, 1)).mean()

    def train():
        model.train()
        optimizer.zero_grad()
        loss = nll_loss(model(), dataset.y)
        loss.backward()
        optimizer.step()
        return loss

    if fanouts is not None:
        # one epoch = the seeds 0 .. num_nodes-1 in batches; every batch samples its blocks with a fresh rng_seed, gathers
        # the features of the first block's source nodes and makes one step on the batch's labels
        from .sampling import NeighborSampler
        sampler = NeighborSampler(inputInfo, fanouts, want_edge_ids=args.edge_dim > 0)      # (the blocks' edge features)
        all_nodes = torch.arange(dataset.num_nodes, dtype=torch.int32, device=device)
        batches = [all_nodes[lo: lo + args.batch_size] for lo in range(0, dataset.num_nodes, args.batch_size)]
        drawn = [0]
        first_loss = [None]
        if capture is not None:
            capture.update(sampler=sampler)

        def train():                                   # noqa: F811  (the mini-batch epoch replaces the full-graph step)
            model.train()
            loss = None
            for seeds in batches:
                blocks, input_nodes = sampler.sample(seeds, 0x5A17 + drawn[0] * len(fanouts))
                drawn[0] += 1
                optimizer.zero_grad()
                loss = nll_loss(model(dataset.x.index_select(0, input_nodes), blocks), dataset.y.index_select(0, seeds))
                loss.backward()
                optimizer.step()
                if first_loss[0] is None:
                    first_loss[0] = float(loss.detach())
                    if verbose_mode:
                        print("# first loss: {:.6f}".format(first_loss[0]))
            return loss

        for _ in range(max(1, -(-10 // len(batches)))):   # dry run: at least 10 steps
            loss = train()
        torch.cuda.synchronize()
        start_train = time.perf_counter()
        for _ in range(1, args.num_epoches + 1):
            loss = train()
        torch.cuda.synchronize()
        train_time = time.perf_counter() - start_train
        if capture is not None:
            capture.update(first_loss=first_loss[0], final_loss=float(loss.detach()))
    elif saint:
        # one epoch = --saint_steps steps; every step walks from fresh roots, cuts the induced subgraph of the visited nodes out on
        # the device (one walk call, one subgraph call), gathers x and y by its nodes and makes one step on ALL its nodes: the
        # layers run on the subgraph as on any graph batch, at full depth
        from .sampling import SaintRWSampler
        sampler = SaintRWSampler(inputInfo, args.saint_roots, args.walk_length, seed=0x5A17)
        if args.saint_coverage > 0:
            sampler.estimate_norms(args.saint_coverage)
        drawn = [0]
        first_loss = [None]
        if capture is not None:
            capture.update(sampler=sampler)

        def saint_logits(x, sub):
            if args.model == 'gin':
                for i, conv in enumerate(model.convs):
                    x = conv(x, sub, relu=i + 1 < len(model.convs))
            elif attention:
                kw = {} if edge_attr is None else dict(edge_attr=edge_attr.index_select(0, sub.edge_ids.long()))
                x = model.conv2(F.elu(model.conv1(x, sub, **kw)), sub, **kw)
            else:
                x = model.conv2(model.conv1(x, sub, relu=True), sub)
            return F.log_softmax(x.float(), dim=1)

        def train():                                   # noqa: F811  (the subgraph epoch replaces the full-graph step)
            model.train()
            loss = None
            for _ in range(args.saint_steps):
                sub = sampler.sample(drawn[0])
                drawn[0] += 1
                rows = sub.nodes.long()
                optimizer.zero_grad()
                log_prob = saint_logits(dataset.x.index_select(0, rows), sub)
                picked = -log_prob.gather(1, dataset.y.index_select(0, rows).view(-1, 1)).view(-1)
                weight = sub.node_weight
                # GraphSAINT's loss normalisation: sum_v L_v / lambda_v over the subgraph, lambda_v = N C_v / T
                loss = picked.mean() if weight is None else (picked * weight).sum()
                loss.backward()
                optimizer.step()
                if first_loss[0] is None:
                    first_loss[0] = float(loss.detach())
                    if verbose_mode:
                        print("# first loss: {:.6f}".format(first_loss[0]))
            return loss

        for _ in range(max(1, -(-10 // args.saint_steps))):   # dry run: at least 10 steps
            loss = train()
        torch.cuda.synchronize()
        start_train = time.perf_counter()
        for _ in range(1, args.num_epoches + 1):
            loss = train()
        torch.cuda.synchronize()
        train_time = time.perf_counter() - start_train
        if capture is not None:
            capture.update(first_loss=first_loss[0], final_loss=float(loss.detach()))
    elif not use_graph:
        for i in range(10):   # dry run
            loss = train()
            if i == 0 and capture is not None:
                capture.update(first_loss=float(loss.detach()))
            if i == 0 and verbose_mode:
                print("# first loss: {:.6f}".format(float(loss)))
        torch.cuda.synchronize()
        start_train = time.perf_counter()
        for _ in range(1, args.num_epoches + 1):
            loss = train()
        torch.cuda.synchronize()
        train_time = time.perf_counter() - start_train
        if capture is not None:
            capture.update(final_loss=float(loss.detach()))
    else:
        # libgnna never synchronises and allocates its per-stream scratch on first use, so the dry runs
        # are made on the capture stream; after them one epoch is recorded and replayed per epoch
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(10):   # dry run
                train()
        side.synchronize()
        epoch_graph = torch.cuda.CUDAGraph()
        optimizer.zero_grad(set_to_none=True)
        with torch.cuda.graph(epoch_graph, stream=side):
            loss = train()
        torch.cuda.synchronize()
        start_train = time.perf_counter()
        for _ in range(1, args.num_epoches + 1):
            epoch_graph.replay()
        torch.cuda.synchronize()
        train_time = time.perf_counter() - start_train
    if verbose_mode:
        print("# final loss: {:.6f}".format(float(loss)))
    print('Time (ms): {:.3f}'.format(train_time * 1e3 / args.num_epoches))
    print()
    return 0


if __name__ == '__main__':
    sys.exit(main())
