"""TEST INFRASTRUCTURE ONLY. Torch-CPU fp64 restatement of the ST-GCN recogniser's forward with a BLOCK PLAN argument, for the graphs and plans
oracle/stgcn_oracle.py (ten blocks, hard-coded) does not state: the six-block extractor of the reference's unconstrained evaluation
(eval/unconstrained/models/stgcn.py:77-114) and any plan rgn_stgcn_set_blocks accepts. Lines followed: STGCN.forward
(eval/a2m/recognition/models/stgcn.py:76-123), st_gcn (:145-228), ConvTemporalGraphical (stgcnutils/tgcn.py:61-71).

Pinned against the reference's own outputs (tests/golden/small_graph_uncond.npz, small_graph_ntu25.npz) and, with the ten-block plan, against
oracle.stgcn_oracle.stgcn_forward (tests/test_small_graph_cpu.py)."""
import numpy as np
import torch
import torch.nn.functional as F

TEN = [(64, 1), (64, 1), (64, 1), (64, 1), (128, 2), (128, 1), (128, 1), (256, 2), (256, 1), (256, 1)]      # stgcn.py:51-62
SIX = [(64, 1), (64, 1), (64, 1), (128, 2), (128, 1), (256, 2)]                                              # eval/unconstrained/models/stgcn.py:52-63
FOUR = [(64, 1), (128, 2), (256, 2), (256, 1)]


def _t(sd, k):
    return torch.from_numpy(np.asarray(sd[k])).double()


def _bn(sd, prefix, x):
    return F.batch_norm(x, _t(sd, prefix + ".running_mean"), _t(sd, prefix + ".running_var"), _t(sd, prefix + ".weight"), _t(sd, prefix + ".bias"),
                        training=False, eps=1e-5)


def tree_graph(V, hub_children, rng):
    """tests/test_eval_gpu.py::_tree_graph: a random skeleton in the reference's 'spatial' partition form; vertex 0 is a hub with `hub_children` children."""
    parent = np.zeros(V, np.int64)
    for v in range(1, V):
        parent[v] = 0 if v <= hub_children else rng.integers(1, v)
    adj = np.eye(V)
    for v in range(1, V):
        adj[v, parent[v]] = adj[parent[v], v] = 1.0
    dn = adj / adj.sum(0, keepdims=True)
    A = np.zeros((3, V, V), np.float32)
    for v in range(V):
        for w in range(V):
            if adj[v, w] == 0:
                continue
            A[0 if v == w else (1 if parent[w] == v else 2), v, w] = dn[v, w]
    return A


def forward(sd, x, blocks=None, num_person=1):
    """x [N, V, C * num_person, T] (batch['output'] / batch['x']) -> (features [N, 256], yhat [N, num_class]), fp64.
    blocks: [(out_channels, stride), ...]; None = TEN. A block has the convolved shortcut exactly when the checkpoint holds it (st_gcn.__init__)."""
    blocks = TEN if blocks is None else blocks
    x = torch.as_tensor(np.asarray(x)).double()
    N, V, C2, T = x.shape
    M = num_person
    C = C2 // M
    x = x.reshape(N, V, M, C, T).permute(0, 2, 1, 3, 4).contiguous().view(N, M * V * C, T)       # stgcn.py:83-95: BatchNorm1d channel (m V + v) C + c
    x = _bn(sd, "data_bn", x)
    x = x.view(N, M, V, C, T).permute(0, 1, 3, 4, 2).contiguous().view(N * M, C, T, V)            # :99-101
    A0 = (_t(sd, "A").float()).double()
    K = A0.shape[0]
    for i, (co, stride) in enumerate(blocks):
        p = f"st_gcn_networks.{i}."
        A = (torch.from_numpy(np.asarray(sd["A"])).float() * torch.from_numpy(np.asarray(sd[f"edge_importance.{i}"])).float()).double()   # :105 (an fp32 product there)
        if i == 0:
            res = 0
        elif (p + "residual.0.weight") in sd:
            res = _bn(sd, p + "residual.1", F.conv2d(x, _t(sd, p + "residual.0.weight"), _t(sd, p + "residual.0.bias"), stride=(stride, 1)))
        else:
            res = x
        y = F.conv2d(x, _t(sd, p + "gcn.conv.weight"), _t(sd, p + "gcn.conv.bias"))
        n, kc, t, v = y.shape
        y = torch.einsum("nkctv,kvw->nctw", y.view(n, K, kc // K, t, v), A)
        y = F.relu(_bn(sd, p + "tcn.0", y))
        y = F.conv2d(y, _t(sd, p + "tcn.2.weight"), _t(sd, p + "tcn.2.bias"), stride=(stride, 1), padding=(4, 0))
        y = _bn(sd, p + "tcn.3", y)
        x = F.relu(y + res)
    assert f"st_gcn_networks.{len(blocks)}.gcn.conv.weight" not in sd, "the checkpoint holds more blocks than the plan"
    x = F.avg_pool2d(x, x.shape[2:])
    x = x.view(N, M, -1, 1, 1).mean(dim=1)
    feats = x.reshape(N, -1)
    yhat = F.conv2d(x, _t(sd, "fcn.weight"), _t(sd, "fcn.bias")).view(N, -1)
    return feats, yhat
