"""Synthetic checkpoints and inputs for the ReGenNet sampling hot path.

No trained checkpoint, dataset or SMPL-X asset exists in the build environment,
so tests and bench.py use a deterministic synthetic checkpoint emitted with the *reference's*
state_dict key names and shapes (model/cmdm.py:53-105 in the reference), and synthetic actor
motions laid out like `ccollate` produces them (data_loaders/tensors.py:57-94): `cmotion`
[B, 56, 6, T] = 55 SMPL-X joints in rot6d + one translation row [tx,ty,tz,0,0,0]
(data_loaders/a2m/dataset.py:175-181).

Everything here is NumPy (PCG64) so it is reproducible on any box without the reference.
"""
import numpy as np

# Named configurations mirroring BASELINE.json `configs`.
CONFIGS = {
    # NTU120-AS shipped config: README.md:96 + utils/parser_util.py defaults + utils/model_util.py:66-72
    "ntu": dict(dataset="ntu", njoints=56, nfeats=6, num_frames=60, latent_dim=512, ff_size=1024,
                num_heads=4, layers=8, cm_mode="concat", cond_mode="no_cond", cond_mask_prob=0.0,
                num_actions=26),
    "ntu_action": dict(dataset="ntu", njoints=56, nfeats=6, num_frames=60, latent_dim=512, ff_size=1024,
                       num_heads=4, layers=8, cm_mode="concat", cond_mode="action", cond_mask_prob=0.1,
                       num_actions=26),
    "chi3d": dict(dataset="chi3d", njoints=56, nfeats=6, num_frames=150, latent_dim=512, ff_size=1024,
                  num_heads=4, layers=8, cm_mode="concat", cond_mode="action", cond_mask_prob=0.1,
                  num_actions=8),
    "text150": dict(dataset="chi3d", njoints=56, nfeats=6, num_frames=150, latent_dim=512, ff_size=1024,
                    num_heads=4, layers=8, cm_mode="concat", cond_mode="text", cond_mask_prob=0.1,
                    num_actions=1),
    # small configs the oracle / reference finish in milliseconds
    "tiny": dict(dataset="ntu", njoints=5, nfeats=6, num_frames=8, latent_dim=64, ff_size=128,
                 num_heads=4, layers=2, cm_mode="concat", cond_mode="action", cond_mask_prob=0.1,
                 num_actions=3),
    "tiny_add": dict(dataset="ntu", njoints=5, nfeats=6, num_frames=8, latent_dim=64, ff_size=128,
                     num_heads=4, layers=2, cm_mode="add", cond_mode="no_cond", cond_mask_prob=0.0,
                     num_actions=1),
    "tiny_text": dict(dataset="ntu", njoints=5, nfeats=6, num_frames=11, latent_dim=64, ff_size=128,
                      num_heads=2, layers=2, cm_mode="concat", cond_mode="text", cond_mask_prob=0.1,
                      num_actions=1),
}
# arch='offline' (model/cmdm.py:228-238): the same shapes with the non-causal encoder denoiser
for _name in ("tiny", "tiny_add", "ntu", "ntu_action", "chi3d"):
    CONFIGS[_name + "_offline"] = dict(CONFIGS[_name], arch="offline")
# arch='mlp' (model/cmdm.py:239-242, model/mlp.py): the same shapes with the DiffMLP time / feature mixer (num_heads / ff_size are not read)
for _name in ("tiny", "tiny_add", "tiny_text", "ntu", "ntu_action", "chi3d"):
    CONFIGS[_name + "_mlp"] = dict(CONFIGS[_name], arch="mlp")
# arch='gru' (model/cmdm.py:191-199, 243-249): the same shapes with the nn.GRU(d, d, layers) denoiser; the reference's gru branch is cm_mode='add' only
for _name in ("tiny", "tiny_add", "tiny_text", "ntu", "ntu_action", "chi3d"):
    CONFIGS[_name + "_gru"] = dict(CONFIGS[_name], arch="gru", cm_mode="add")
del _name


def get_config(name, **overrides):
    cfg = dict(CONFIGS[name])
    cfg.update(overrides)
    return cfg


def positional_table(d_model, max_len=5000):
    """Sinusoid table [max_len, 1, d] exactly as PositionalEncoding builds it (model/cmdm.py:269-276):
    fp32 arithmetic throughout (torch.arange(...).float(), torch.exp, torch.sin/cos on fp32)."""
    position = np.arange(0, max_len, dtype=np.float32)[:, None]
    div_term = np.exp(np.arange(0, d_model, 2, dtype=np.float32) * np.float32(-np.log(10000.0) / d_model))
    div_term = div_term.astype(np.float32)
    pe = np.zeros((max_len, d_model), dtype=np.float32)
    ang = (position * div_term).astype(np.float32)
    pe[:, 0::2] = np.sin(ang)
    pe[:, 1::2] = np.cos(ang)
    return pe[:, None, :]


def make_state_dict(cfg, seed=0):
    """Deterministic synthetic checkpoint: dict key -> float32 ndarray, reference key names.

    Linear weights ~ N(0, gain^2/fan_in); q/k projections get a larger gain so the causal softmax is
    far from uniform; LayerNorm gamma ~ 1+0.1N, beta ~ 0.1N; biases ~ 0.02..0.1 N.
    cfg["arch"] == "offline": nn.TransformerEncoderLayer keys (seqTransEncoder.layers.<l>: self_attn, linear1/2, norm1/2) drawn
    in the decoder's order without the cross-attention and norm3 draws, q/k at gain 1; every other config draws exactly what it always did.
    cfg["arch"] == "mlp": DiffMLP keys (mlp.motion_mlp.mlps.<l>: conct in block 0, fc0 [T, T, 1], fc1, emb_fc, norm0/1). The stack adds 2 L
    un-normalised SiLU branches to the stream and ends in no LayerNorm, so the branch weights are drawn at a gain (MLP_GAIN) and the output
    projection at one (MLP_OUT_GAIN) that keep the denoiser's outputs O(1): an absolute parity bound means nothing on a stream that has blown up.
    cfg["arch"] == "gru": both pose embeddings read [pose ; emb] (F + d columns) and the layers are nn.GRU's keys (gru.weight_ih_l<k>, weight_hh_l<k>
    [3d, d], bias_ih_l<k>, bias_hh_l<k> [3d], gate order r, z, n). The state lives in (-1, 1), so the recurrent and input weights are drawn at a gain
    (GRU_GAIN) at which the state carries through the scan - the gates neither sit at 1/2 nor saturate - and the output projection at one
    (GRU_OUT_GAIN) that puts the recorded outputs' max-abs in [1, 4].
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    d, ff, L = cfg["latent_dim"], cfg["ff_size"], cfg["layers"]
    F = cfg["njoints"] * cfg["nfeats"]
    sd = {}

    def lin(prefix, out_f, in_f, gain=1.0, bias_std=0.05):
        sd[prefix + ".weight"] = (rng.standard_normal((out_f, in_f)) * (gain / np.sqrt(in_f))).astype(np.float32)
        sd[prefix + ".bias"] = (rng.standard_normal(out_f) * bias_std).astype(np.float32)

    gru = cfg.get("arch", "online") == "gru"
    lin("input_process.poseEmbedding", d, F + (d if gru else 0))
    lin("cmo_process.poseEmbedding", d, F + (d if gru else 0))
    if cfg["cm_mode"] == "concat":
        lin("fuse_process", d, 2 * d, gain=1.4)
    pe = positional_table(d)
    sd["sequence_pos_encoder.pe"] = pe
    sd["embed_timestep.sequence_pos_encoder.pe"] = pe.copy()
    lin("embed_timestep.time_embed.0", d, d, gain=1.5)
    lin("embed_timestep.time_embed.2", d, d, gain=1.5)
    enc = cfg.get("arch", "online") == "offline"
    mix = cfg.get("arch", "online") == "mlp"
    for l in range(L if mix else 0):
        p = f"mlp.motion_mlp.mlps.{l}."
        T = cfg["num_frames"]
        if l == 0:
            lin(p + "conct", d, 2 * d, gain=1.4)
        sd[p + "fc0.weight"] = (rng.standard_normal((T, T, 1)) * (MLP_GAIN / np.sqrt(T))).astype(np.float32)
        sd[p + "fc0.bias"] = (rng.standard_normal(T) * 0.05).astype(np.float32)
        lin(p + "fc1", d, d, gain=MLP_GAIN)
        lin(p + "emb_fc", d, d, gain=0.5)
        for n in ("norm0", "norm1"):
            sd[p + n + ".weight"] = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
            sd[p + n + ".bias"] = (0.1 * rng.standard_normal(d)).astype(np.float32)
    for l in range(L if gru else 0):
        for part in ("ih", "hh"):
            sd[f"gru.weight_{part}_l{l}"] = (rng.standard_normal((3 * d, d)) * (GRU_GAIN / np.sqrt(d))).astype(np.float32)
        for part in ("ih", "hh"):
            sd[f"gru.bias_{part}_l{l}"] = (rng.standard_normal(3 * d) * 0.05).astype(np.float32)
    for l in range(0 if (mix or gru) else L):
        p = f"seqTransEncoder.layers.{l}." if enc else f"seqTransDecoder.layers.{l}."
        w = rng.standard_normal((3 * d, d)) / np.sqrt(d)
        # q,k gain -> peaky attention (the encoder's milder: without the decoder's third LayerNorm per layer and its causal
        # mask, 2.5 makes the synthetic offline model so sensitive that fp32 summation order alone moves guided loops by 1e-1)
        w[: 2 * d] *= 1.0 if enc else 2.5
        sd[p + "self_attn.in_proj_weight"] = w.astype(np.float32)
        sd[p + "self_attn.in_proj_bias"] = (rng.standard_normal(3 * d) * 0.05).astype(np.float32)
        lin(p + "self_attn.out_proj", d, d)
        if not enc:
            sd[p + "multihead_attn.in_proj_weight"] = (rng.standard_normal((3 * d, d)) / np.sqrt(d)).astype(np.float32)
            sd[p + "multihead_attn.in_proj_bias"] = (rng.standard_normal(3 * d) * 0.05).astype(np.float32)
            lin(p + "multihead_attn.out_proj", d, d)
        lin(p + "linear1", ff, d, gain=1.2)
        lin(p + "linear2", d, ff, gain=1.2)
        for n in (("norm1", "norm2") if enc else ("norm1", "norm2", "norm3")):
            sd[p + n + ".weight"] = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
            sd[p + n + ".bias"] = (0.1 * rng.standard_normal(d)).astype(np.float32)
    if "text" in cfg["cond_mode"]:
        lin("embed_text", d, cfg.get("clip_dim", 512))
    if "action" in cfg["cond_mode"]:
        sd["embed_action.action_embedding"] = rng.standard_normal((cfg["num_actions"], d)).astype(np.float32)
    lin("output_process.poseFinal", F, d, gain=MLP_OUT_GAIN / L if mix else (GRU_OUT_GAIN if gru else 1.0))
    return sd


MLP_GAIN, MLP_OUT_GAIN = 1.0, 0.8   # (the projection gain is MLP_OUT_GAIN / layers: the stream grows with every block)
GRU_GAIN, GRU_OUT_GAIN = 1.5, 1.0   # (tests/golden/make_golden_gru_arch.py asserts the output range; tests/test_gru_arch_cpu.py that the recurrence matters)


FAMILIES = ("heavy_tailed", "outlier_channels", "peaky_attention", "big_output", "small_signal", "hostile")


def make_state_dict_family(cfg, family, seed=0):
    """Stress families of synthetic checkpoints for the precision claims (tests: test_stress_family_checkpoints). The i.i.d.-Gaussian
    default above is one point in checkpoint space; trained transformers differ from it in known ways, each of which moves rounding
    error differently: heavy-tailed weights (a few large products dominate a dot product), outlier channels with large LayerNorm gains (the
    'massive activation' channels: an operand's rounding is relative, so a large channel carries a large absolute error into every GEMM that
    reads it), near-one-hot attention (scores far apart: the softmax amplifies score error), a high-gain output projection (multiplies whatever
    error the last layer carries) and a small-signal model (everything near the LayerNorm epsilon's regime). Each is the default checkpoint of
    `seed` with one transformation, so the reference key set and shapes are unchanged. "hostile" stacks them until plain 16-bit operands are
    not enough: the checkpoint the calibration's refusal path is tested with."""
    sd = make_state_dict(cfg, seed=seed)
    if family in (None, "", "gaussian"):
        return sd
    rng = np.random.Generator(np.random.PCG64(7919 + seed))
    d, L = cfg["latent_dim"], cfg["layers"]
    lin_keys = [k for k in sd if k.endswith(".weight") and sd[k].ndim == 2 and "norm" not in k] + [k for k in sd if k.endswith("in_proj_weight")]
    ln_keys = [k for k in sd if ".norm" in k and k.endswith(".weight")]

    def heavy():
        for k in lin_keys:   # Student-t, nu = 3, at the row scale of the Gaussian draw it replaces
            w = sd[k]
            row = w.std(axis=1, keepdims=True)
            sd[k] = (rng.standard_t(3, w.shape) / np.sqrt(3.0) * row).astype(np.float32)

    def outliers(n, gain, compensate):
        # LayerNorm gain AND shift x gain on n channels of every norm: the residual stream carries a few channels `gain` times larger than the rest
        # (they dominate the next LayerNorm's statistics). compensate: the weights that READ those channels - linear1 behind norm2, the next
        # layer's in_proj / the output projection behind norm3 - are 1 / gain there, as training leaves them (the sub-layers then see O(1)
        # inputs). Without it the denoiser's gain is so large that the sampling loop is a chaotic map: see test_parity_presupposes_...
        ch = rng.choice(d, size=n, replace=False)
        for k in ln_keys:
            for kk in (k, k[: -len("weight")] + "bias"):
                g = sd[kk].copy()
                g[ch] *= gain
                sd[kk] = g
        if compensate:
            readers = [f"seqTransDecoder.layers.{l}.linear1.weight" for l in range(L)] + \
                      [f"seqTransDecoder.layers.{l}.self_attn.in_proj_weight" for l in range(1, L)] + ["output_process.poseFinal.weight"]
            for k in readers:
                w = sd[k].copy()
                w[:, ch] /= gain
                sd[k] = w

    def peaky(gain):
        for l in range(L):
            k = f"seqTransDecoder.layers.{l}.self_attn.in_proj_weight"
            w = sd[k].copy()
            w[: 2 * d] *= gain / 2.5
            sd[k] = w

    if family == "heavy_tailed":
        heavy()
    elif family == "outlier_channels":
        outliers(6, 2.0, True)
    elif family == "outlier_channels_uncompensated":
        outliers(6, 8.0, False)
    elif family == "peaky_attention":
        peaky(6.0)
    elif family == "big_output":
        sd["output_process.poseFinal.weight"] = sd["output_process.poseFinal.weight"] * np.float32(3.0)
    elif family == "small_signal":
        for k in lin_keys:
            sd[k] = sd[k] * np.float32(0.3)
    elif family == "hostile":
        heavy()
        outliers(24, 64.0, False)
        peaky(10.0)
        sd["output_process.poseFinal.weight"] = sd["output_process.poseFinal.weight"] * np.float32(8.0)
    else:
        raise ValueError(f"unknown checkpoint family {family!r}: {FAMILIES}")
    return sd


def _random_rot6d(rng, shape):
    """rot6d (first two rows of a rotation matrix, row-major) of uniformly random rotations."""
    q = rng.standard_normal(shape + (4,))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    r0 = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1)
    r1 = np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1)
    return np.concatenate([r0, r1], -1)


def make_cmotion(cfg, batch, seed=1):
    """Actor motion [B, njoints, 6, T] fp32: rot6d joints + last row = translation [tx,ty,tz,0,0,0].
    Other feature layouts (nfeats != 6, e.g. a 263 x 1 feature vector): [B, njoints, nfeats, T] ~ N(0, 1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    J, T = cfg["njoints"], cfg["num_frames"]
    if cfg["nfeats"] != 6:
        return rng.standard_normal((batch, J, cfg["nfeats"], T)).astype(np.float32)
    rot = _random_rot6d(rng, (batch, T, J - 1))                   # [B,T,J-1,6]
    tr = np.zeros((batch, T, 1, 6))
    tr[..., 0, :3] = rng.uniform(-1, 1, (batch, T, 3))
    cm = np.concatenate([rot, tr], axis=2)                          # [B,T,J,6]
    return np.ascontiguousarray(cm.transpose(0, 2, 3, 1)).astype(np.float32)


def make_noise_tape(cfg, batch, steps, seed=10):
    """[steps+1, B, J, 6, T] fp32 N(0,1): entry 0 is x_T, entry k the k-th per-step draw."""
    rng = np.random.Generator(np.random.PCG64(seed))
    shape = (steps + 1, batch, cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    return rng.standard_normal(shape, dtype=np.float32)


def make_actions(cfg, batch, seed=2):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, max(cfg["num_actions"], 1), (batch, 1)).astype(np.int64)


def make_text_features(cfg, batch, seed=3):
    """Stand-in for CLIP ViT-B/32 text features [B, 512] (CLIP itself is out of scope)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = rng.standard_normal((batch, cfg.get("clip_dim", 512)))
    f /= np.linalg.norm(f, axis=-1, keepdims=True)
    return f.astype(np.float32)


def make_stgcn_graph(V=56):
    """A synthetic skeleton in the reference's 'spatial' partition form (stgcnutils/graph.py): a binary tree over V joints; A[0] self loops, A[1] the
    edge from the parent, A[2] the edges from the children, column-normalised. For tools that need a recogniser without the reference's graph file."""
    parent = [(v - 1) // 2 for v in range(V)]
    adj = np.eye(V)
    for v in range(1, V):
        adj[v, parent[v]] = adj[parent[v], v] = 1.0
    dn = adj / adj.sum(0, keepdims=True)
    A = np.zeros((3, V, V), np.float32)
    for v in range(V):
        for w in range(V):
            if adj[v, w]:
                A[0 if v == w else (1 if parent[w] == v else 2), v, w] = dn[v, w]
    return A


def make_stgcn_state_dict(A, num_class=26, in_channels=12, num_person=2, seed=0, blocks=None):
    """Synthetic checkpoint of the ST-GCN evaluator with the reference's state_dict keys
    (eval/a2m/recognition/models/stgcn.py:44-73,183-219; stgcnutils/tgcn.py:51-59). `A` [K, V, V] is the adjacency buffer
    the reference registers (stgcn.py:42); BatchNorm running statistics are non-trivial so that folding them is exercised.
    blocks: [(out_channels, stride), ...], None = the ten blocks of stgcn.py:51-62 (the draws of the default do not change); the six of
    eval/unconstrained/models/stgcn.py:52-63 are regennet_amd.eval.stgcn.SIX_BLOCKS."""
    rng = np.random.Generator(np.random.PCG64(seed))
    K, V = int(A.shape[0]), int(A.shape[1])
    sd = {"A": np.asarray(A, dtype=np.float32)}

    def bn(prefix, c):
        sd[prefix + ".weight"] = (1.0 + 0.2 * rng.standard_normal(c)).astype(np.float32)
        sd[prefix + ".bias"] = (0.1 * rng.standard_normal(c)).astype(np.float32)
        sd[prefix + ".running_mean"] = (0.2 * rng.standard_normal(c)).astype(np.float32)
        sd[prefix + ".running_var"] = rng.uniform(0.5, 1.5, c).astype(np.float32)
        sd[prefix + ".num_batches_tracked"] = np.array(100, dtype=np.int64)

    def conv(prefix, co, ci, kt, gain=1.0):
        sd[prefix + ".weight"] = (rng.standard_normal((co, ci, kt, 1)) * (gain / np.sqrt(ci * kt))).astype(np.float32)
        sd[prefix + ".bias"] = (0.05 * rng.standard_normal(co)).astype(np.float32)

    bn("data_bn", in_channels * V)
    chans = [(in_channels // num_person, 64, 1), (64, 64, 1), (64, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 1), (128, 128, 1),
             (128, 256, 2), (256, 256, 1), (256, 256, 1)]
    if blocks is not None:
        chans = [(in_channels // num_person if i == 0 else blocks[i - 1][0], co, st) for i, (co, st) in enumerate(blocks)]
    for i, (ci, co, stride) in enumerate(chans):
        p = f"st_gcn_networks.{i}."
        conv(p + "gcn.conv", co * K, ci, 1, gain=1.5)
        bn(p + "tcn.0", co)
        conv(p + "tcn.2", co, co, 9, gain=1.5)
        bn(p + "tcn.3", co)
        if i > 0 and (ci != co or stride != 1):
            conv(p + "residual.0", co, ci, 1)
            bn(p + "residual.1", co)
        sd[f"edge_importance.{i}"] = (1.0 + 0.3 * rng.standard_normal((K, V, V))).astype(np.float32)
    conv("fcn", num_class, 256, 1)
    return sd


def make_gru_state_dict(input_size=72, hidden=128, layers=2, lin1=30, num_classes=12, seed=0, scale=1.0):
    """Synthetic checkpoint of the GRU action classifier with the reference's state_dict keys (eval/a2m/action2motion/models.py:15-17: nn.GRU ->
    Linear(hidden, 30) -> Linear(30, classes)): every tensor uniform in PyTorch's default init range (+-1/sqrt(hidden) for the GRU, +-1/sqrt(fan_in)
    for the Linears) times `scale` (scale > 1 drives the gates into saturation)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}

    def uni(shape, bound):
        return (rng.uniform(-bound, bound, shape) * scale).astype(np.float32)

    kg = 1.0 / np.sqrt(hidden)
    for l in range(layers):
        sd[f"recurrent.weight_ih_l{l}"] = uni((3 * hidden, input_size if l == 0 else hidden), kg)
        sd[f"recurrent.weight_hh_l{l}"] = uni((3 * hidden, hidden), kg)
        sd[f"recurrent.bias_ih_l{l}"] = uni((3 * hidden,), kg)
        sd[f"recurrent.bias_hh_l{l}"] = uni((3 * hidden,), kg)
    sd["linear1.weight"] = uni((lin1, hidden), kg)
    sd["linear1.bias"] = uni((lin1,), kg)
    sd["linear2.weight"] = uni((num_classes, lin1), 1.0 / np.sqrt(lin1))
    sd["linear2.bias"] = uni((num_classes,), 1.0 / np.sqrt(lin1))
    return sd


def make_gru_inputs(N, input_size, T, hidden=128, layers=2, seed=0, lengths="mixed", nfeats=3):
    """Inputs of the GRU classifier: (x [N, input_size / nfeats, nfeats, T] like batch['output_xyz'] (nfeats falls back to 1 when it does not divide
    input_size), lengths int64 [N], hidden_unit [layers, N, hidden]). lengths: "full" (all T), "mixed" (uniform in [1, T], row 0 = 1 and row 1 = T
    where there are such rows) or an explicit list."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if input_size % nfeats:
        nfeats = 1
    x = rng.standard_normal((N, input_size // nfeats, nfeats, T)).astype(np.float32)
    h0 = rng.standard_normal((layers, N, hidden)).astype(np.float32)
    if isinstance(lengths, str):
        if lengths == "full":
            ln = np.full(N, T, np.int64)
        else:
            ln = rng.integers(1, T + 1, N).astype(np.int64)
            ln[0] = 1
            if N > 1:
                ln[1] = T
    else:
        ln = np.asarray(lengths, np.int64)
    return x, ln, h0


def make_t2m_state_dicts(dim_pose=263, movement_hidden=512, movement_latent=512, motion_hidden=1024, dim_word=300, dim_pos_ohot=15, text_hidden=512,
                         coemb=512, seed=0, scale=1.0, out_scale=1.0):
    """Synthetic checkpoint of the text-to-motion evaluator, shaped like the reference's finest.tar: {'movement_encoder': {...}, 'text_encoder': {...},
    'motion_encoder': {...}} with the state_dict keys of data_loaders/humanml/networks/modules.py (MovementConvEncoder, TextEncoderBiGRUCo,
    MotionEncoderBiGRUCo). Tensors are uniform in PyTorch's default init range times `scale` (scale > 1 drives the gates into saturation); `hidden` is
    normal; the LayerNorm's affine is near (1, 0); the last Linear of each head takes `out_scale` instead, so the embeddings keep their size."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def uni(shape, fan_in, sc=None):
        b = 1.0 / np.sqrt(fan_in)
        return (rng.uniform(-b, b, shape) * (scale if sc is None else sc)).astype(np.float32)

    C = dim_pose - 4
    mov = {"main.0.weight": uni((movement_hidden, C, 4), 4 * C), "main.0.bias": uni((movement_hidden,), 4 * C),
           "main.3.weight": uni((movement_latent, movement_hidden, 4), 4 * movement_hidden), "main.3.bias": uni((movement_latent,), 4 * movement_hidden),
           "out_net.weight": uni((movement_latent, movement_latent), movement_latent), "out_net.bias": uni((movement_latent,), movement_latent)}

    def bigru(H, sd):
        for sfx in ("_l0", "_l0_reverse"):
            sd["gru.weight_ih" + sfx] = uni((3 * H, H), H)
            sd["gru.weight_hh" + sfx] = uni((3 * H, H), H)
            sd["gru.bias_ih" + sfx] = uni((3 * H,), H)
            sd["gru.bias_hh" + sfx] = uni((3 * H,), H)
        sd["output_net.0.weight"] = uni((H, 2 * H), 2 * H)
        sd["output_net.0.bias"] = uni((H,), 2 * H)
        sd["output_net.1.weight"] = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
        sd["output_net.1.bias"] = (0.1 * rng.standard_normal(H)).astype(np.float32)
        sd["output_net.3.weight"] = uni((coemb, H), H, out_scale)
        sd["output_net.3.bias"] = uni((coemb,), H, out_scale)
        sd["hidden"] = rng.standard_normal((2, 1, H)).astype(np.float32)
        return sd

    text = bigru(text_hidden, {"pos_emb.weight": uni((dim_word, dim_pos_ohot), dim_pos_ohot), "pos_emb.bias": uni((dim_word,), dim_pos_ohot),
                               "input_emb.weight": uni((text_hidden, dim_word), dim_word), "input_emb.bias": uni((text_hidden,), dim_word)})
    motion = bigru(motion_hidden, {"input_emb.weight": uni((motion_hidden, movement_latent), movement_latent),
                                   "input_emb.bias": uni((motion_hidden,), movement_latent)})
    return {"movement_encoder": mov, "text_encoder": text, "motion_encoder": motion}


def make_t2m_inputs(N, T, Lw, seed=0, lengths="mixed", dim_pose=263, dim_word=300, dim_pos_ohot=15):
    """Inputs of the text-to-motion evaluator as eval_humanml's batches carry them: {'motions' [N, T, dim_pose], 'm_lens' int64 [N] in [4, T],
    'word_embs' [N, Lw, dim_word], 'pos_ohot' [N, Lw, dim_pos_ohot] one-hot, 'cap_lens' int64 [N] in [1, Lw]}. lengths: "full", "mixed" (m_lens
    uniform in [4, T] with T, 40, 4, 41, 42 and 43 among the first rows where they fit; cap_lens cycling 1 .. Lw) or a (m_lens, cap_lens) pair."""
    rng = np.random.Generator(np.random.PCG64(seed))
    motions = rng.standard_normal((N, T, dim_pose)).astype(np.float32)
    word_embs = rng.standard_normal((N, Lw, dim_word)).astype(np.float32)
    pos = rng.integers(0, dim_pos_ohot, (N, Lw))
    pos_ohot = np.zeros((N, Lw, dim_pos_ohot), np.float32)
    np.put_along_axis(pos_ohot, pos[..., None], 1.0, axis=2)
    if isinstance(lengths, str):
        if lengths == "full":
            m_lens, cap_lens = np.full(N, T, np.int64), np.full(N, Lw, np.int64)
        else:
            m_lens = rng.integers(min(4, T), T + 1, N).astype(np.int64)
            for i, v in enumerate(v for v in (T, 40, 4, 41, 42, 43) if 4 <= v <= T):
                if i < N:
                    m_lens[i] = v
            cap_lens = (np.arange(N) % Lw + 1).astype(np.int64)
    else:
        m_lens, cap_lens = (np.asarray(v, np.int64) for v in lengths)
    return {"motions": motions, "m_lens": m_lens, "word_embs": word_embs, "pos_ohot": pos_ohot, "cap_lens": cap_lens}


def build_model(cfg, sd, resp="", precision=None, device="cuda:0", noise_schedule="cosine", sigma_small=True, x3_tail=None, engine_options=None, f16_steps=None):
    """(model, diffusion) from regennet_amd for a synth config + checkpoint dict (reference key names): the same
    constructor calls the reference factory makes (utils/model_util.py:66-117), for tests, bench.py and tools.
    x3_tail=None here means the engine's default rule — it was derived on exactly these synthetic checkpoints;
    a model that loads a checkpoint through the plain factory path measures its switch point instead ("auto")."""
    import torch

    from .diffusion import gaussian_diffusion as gd
    from .diffusion.respace import SpacedDiffusion, space_timesteps
    from .model.cmdm import CMDM
    from .utils.model_util import load_model_wo_clip

    kw = {} if precision is None else {"precision": precision}
    model = CMDM("", cfg["njoints"], cfg["nfeats"], cfg["num_actions"], True, "rot6d", True, True,
                 num_frames=cfg["num_frames"], latent_dim=cfg["latent_dim"], ff_size=cfg["ff_size"],
                 num_layers=cfg["layers"], num_heads=cfg["num_heads"], dropout=0.1, activation="gelu",
                 data_rep="rot6d", dataset=cfg["dataset"], arch=cfg.get("arch", "online"), cm_mode=cfg["cm_mode"], body_model="smplx",
                 cond_mode=cfg["cond_mode"], cond_mask_prob=cfg["cond_mask_prob"], action_emb="tensor",
                 emb_trans_dec=cfg.get("emb_trans_dec", False), wo_pos_emb=cfg.get("wo_pos_emb", False), clip_dim=cfg.get("clip_dim", 512),
                 x3_tail=x3_tail, engine_options=engine_options, f16_steps=f16_steps, **kw)
    load_model_wo_clip(model, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.x3_tail = x3_tail
    model.to(device)
    model.eval()
    diffusion = SpacedDiffusion(use_timesteps=space_timesteps(1000, resp or [1000]),
                                betas=gd.get_named_beta_schedule(noise_schedule, 1000, 1.0),
                                model_mean_type=gd.ModelMeanType.START_X,
                                model_var_type=gd.ModelVarType.FIXED_SMALL if sigma_small else gd.ModelVarType.FIXED_LARGE,
                                loss_type=gd.LossType.MSE, rescale_timesteps=False)
    return model, diffusion


def make_skeleton(njoints=55, depth=10, nbetas=10, seed=0):
    """A deterministic SYNTHETIC skeleton for tests, tools and `--skeleton synthetic`: a valid tree of `njoints` joints in index order
    (parents[0] = -1, parents[i] < i) whose deepest joint is `depth` edges from the root, bones of 5 - 30 cm, and small shape directions.
    Joints 22 - 24 are leaves, as the jaw and the eyes are in SMPL-X: the reference does not hand their rotations to the body layer
    (model/rotation2xyz.py:294-301), which is only harmless because no position depends on them.
    It has the joint count of a body model's skeleton (55 like SMPL-X, 24 like SMPL) and nothing else of it: the licensed models' rest
    joints come from tools/make_skeleton.py. Keys as model/rotation2xyz.py load_skeleton returns them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    J = int(njoints)
    depth = min(int(depth), J - 1)
    parents = np.full(J, -1, dtype=np.int32)
    level = np.zeros(J, dtype=np.int64)
    for i in range(1, J):
        if i <= depth:
            parents[i] = i - 1                                        # a spine of `depth` edges ...
        else:
            ok = level[:i] < depth                                    # ... and every other joint below a joint that is not at the deepest level
            ok[22:25] = False
            parents[i] = rng.choice(np.flatnonzero(ok))
        level[i] = level[parents[i]] + 1
    rest = np.zeros((J, 3))
    rest[0] = rng.uniform(-0.05, 0.05, 3)
    for i in range(1, J):
        d = rng.standard_normal(3)
        rest[i] = rest[parents[i]] + d / np.linalg.norm(d) * rng.uniform(0.05, 0.30)
    return {"rest_joints": rest.astype(np.float32), "parents": parents,
            "shape_joints": (0.01 * rng.standard_normal((J, 3, int(nbetas)))).astype(np.float32), "body_model": f"synthetic{J}"}


def make_body(njoints=55, nverts=130, nbetas=10, seed=0, identity_joints=None):
    """A deterministic SYNTHETIC body for tests, tools and `--skeleton synthetic --vertices`: the skeleton of make_skeleton(njoints, nbetas=nbetas,
    seed=seed), unchanged, under a surface of `nverts` vertices, as model/rotation2xyz.py check_body returns a body file (skeleton keys + 'mesh').
      v_template       within 10 cm of a bone (the segment joint - parent; of the joint itself where there is one joint)
      lbs_weights      four non-zero weights per vertex (fewer where the tree has fewer joints): the bone's joint, its parent and neighbours, normalised
      posedirs         0.01 N(0, 1)
      J_regressor      (mesh['J_regressor'], for tests; no file holds it) synthetic and row-stochastic: with V >= 2 J joint j is the midpoint of
                       vertices 2 j and 2 j + 1, which lie opposite each other about it; with J <= V < 2 J vertex j sits on joint j
      shapedirs        0.005 N(0, 1), then shifted on each joint's own vertices so that J_regressor @ shapedirs IS the skeleton's shape_joints:
                       with J_regressor @ v_template = rest_joints, the rest joints of any betas are the regressor applied to v_shaped
      faces            a triangle strip over the vertex order
      identity_joints  default 22 - 24 for 55 joints (the jaw and eyes Rotation2xyz_x does not hand over), else none
    With fewer vertices than joints there is no such regressor: shapedirs are then plain noise and mesh['J_regressor'] is None.
    It has a body model's array shapes and nothing else of one."""
    sk = make_skeleton(njoints, nbetas=nbetas, seed=seed)
    rng = np.random.Generator(np.random.PCG64([seed, 0x6d657368]))
    J, V, nb = int(njoints), int(nverts), int(nbetas)
    rest, parents = sk["rest_joints"].astype(np.float64), sk["parents"]
    per = 2 if V >= 2 * J else (1 if V >= J else 0)                                # regressor vertices per joint, in front of the others
    bone = rng.integers(1, J, V) if J > 1 else np.zeros(V, np.int64)              # the joint at the far end of the vertex's bone
    bone[:per * J] = np.repeat(np.arange(J), per)
    near = np.maximum(parents[bone], 0)
    s = rng.uniform(0, 1, (V, 1))
    d = rng.standard_normal((V, 3))
    d *= rng.uniform(0, 0.10, (V, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    vt = rest[near] * (1 - s) + rest[bone] * s + d
    if per == 2:
        vt[0:2 * J:2], vt[1:2 * J:2] = rest + d[0:2 * J:2], rest - d[0:2 * J:2]
    elif per == 1:
        vt[:J] = rest
    children = [[int(c) for c in np.flatnonzero(parents == j)] for j in range(J)]
    w = np.zeros((V, J))
    for v in range(V):
        b, n = int(bone[v]), int(near[v])
        group = list(dict.fromkeys([b, n, int(max(parents[n], 0))] + children[b] + children[n]))[:4]
        for j in range(J):                                                         # (a small tree: fill up to four with the lowest free joints)
            if len(group) >= min(4, J):
                break
            if j not in group:
                group.append(j)
        w[v, group] = rng.uniform(0.1, 1.0, len(group))
    w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    posedirs = (0.01 * rng.standard_normal((9 * (J - 1), 3 * V))).astype(np.float32)
    reg = None
    if per:
        reg = np.zeros((J, V))
        for k in range(per):
            reg[np.arange(J), per * np.arange(J) + k] = 1.0 / per
    mesh = {"v_template": vt.astype(np.float32), "posedirs": posedirs, "lbs_weights": w, "shapedirs": None, "J_regressor": reg,
            "faces": np.stack([np.arange(0, V - 2), np.arange(1, V - 1), np.arange(2, V)], 1).astype(np.int32) if V >= 3 else np.zeros((0, 3), np.int32),
            "identity_joints": np.asarray(([22, 23, 24] if J == 55 else []) if identity_joints is None else identity_joints, dtype=np.int32).reshape(-1)}
    if nb > 0:
        sd = 0.005 * rng.standard_normal((V, 3, nb))
        if per:                                                                    # every vertex of joint j takes the same shift: the row's weights sum to 1
            sd[:per * J] += np.repeat(sk["shape_joints"].astype(np.float64) - np.einsum("jv,vck->jck", reg, sd), per, axis=0)
        mesh["shapedirs"] = sd.astype(np.float32)
    sk["mesh"] = mesh
    return sk


def make_joint_regressors(body, npicks=21, nreg=9, support=6, seed=0):
    """Deterministic SYNTHETIC vertex joints, extra-joint regressor and joint-type maps for a body of make_body (or any body dict), as a body file
    holds them beside the mesh (model/rotation2xyz.py check_joint_regressors): body['mesh'].update(make_joint_regressors(body)) attaches them.
      vertex_joints      `npicks` distinct vertices (fewer where the body has fewer)
      J_regressor_extra  [nreg, V]: `support` non-zero weights of mixed sign per row, on random vertices
      joint_maps         index maps into [J chain joints | picked | regressed] with the reference's lengths - vibe 49, a2m 18 of vibe's entries,
                         a2mpl the sorted union of a2m with the first 24 chain joints - drawn to reach all three blocks and to repeat indices
      map_roots          the subtracted output row: vibe 8, a2m 0, a2mpl 0; in all three that row is chain joint 0
    They have the shapes of a body model's tables and nothing else of them: the licensed ones come from tools/make_skeleton.py."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x6a726567]))
    V, J = int(body["mesh"]["v_template"].shape[0]), len(body["parents"])
    Np, Jr, sup = min(int(npicks), V), int(nreg), min(int(support), V)
    picks = np.sort(rng.choice(V, Np, replace=False)).astype(np.int32) if Np else np.zeros(0, np.int32)
    picks = picks[rng.permutation(Np)] if Np else picks
    reg = np.zeros((Jr, V), np.float32)
    for r in range(Jr):
        cols = rng.choice(V, sup, replace=False)
        sign = np.where((np.arange(sup) + rng.integers(0, 2)) % 2 == 0, 1.0, -1.0)
        reg[r, cols] = (sign * rng.uniform(0.2, 1.0, sup)).astype(np.float32)
    nall = J + Np + Jr
    vibe = rng.integers(0, nall, 49)
    vibe[[0, 1, 2]] = [J - 1, min(J, nall - 1), nall - 1]            # the last chain joint, the first and the last joint behind the chain
    vibe[8], vibe[48] = 0, vibe[3]                                  # the root row is chain joint 0; one repeat for certain
    a2m = vibe[np.r_[8, 0, 1, 2, np.sort(rng.choice(np.arange(9, 49), 14, replace=False))]]
    a2mpl = np.unique(np.r_[np.arange(min(24, J)), a2m])
    return {"vertex_joints": picks, "J_regressor_extra": reg,
            "joint_maps": {"vibe": vibe.astype(np.int32), "a2m": a2m.astype(np.int32), "a2mpl": a2mpl.astype(np.int32)},
            "map_roots": {"vibe": 8, "a2m": 0, "a2mpl": 0}}
