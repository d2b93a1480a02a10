"""CMDM denoiser object for arch='online' and arch='offline' — host-side mirror of the reference's `model/cmdm.py`.

The class keeps the reference's constructor keywords, attribute names and state_dict key names
(so `load_model_wo_clip`, `model.to(dev())`, `model.eval()`, `next(model.parameters()).device`,
`model(x, t, y=...)` behave as callers of the reference expect), but it holds the
parameters only as a checkpoint container: `forward` hands the tensors to libregennet_hip.so, where
the whole evaluation (cmdm.py:173-252) runs as HIP kernels. There is no eager/CPU fallback.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..utils import dist_util


class _Pose(nn.Module):          # InputProcess / OutputProcess parameter holders (cmdm.py:301-355)
    def __init__(self, name, fin, fout):
        super().__init__()
        setattr(self, name, nn.Linear(fin, fout))


class _MHA(nn.Module):           # nn.MultiheadAttention's parameter names
    def __init__(self, d):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d, d))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d))
        self.out_proj = nn.Linear(d, d)
        nn.init.xavier_uniform_(self.in_proj_weight)


class _DecoderLayer(nn.Module):  # nn.TransformerDecoderLayer's parameter names
    def __init__(self, d, ff):
        super().__init__()
        self.self_attn = _MHA(d)
        self.multihead_attn = _MHA(d)
        self.linear1 = nn.Linear(d, ff)
        self.linear2 = nn.Linear(ff, d)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(d), nn.LayerNorm(d), nn.LayerNorm(d)


class _Decoder(nn.Module):
    def __init__(self, d, ff, n):
        super().__init__()
        self.layers = nn.ModuleList([_DecoderLayer(d, ff) for _ in range(n)])


class _EncoderLayer(nn.Module):  # nn.TransformerEncoderLayer's parameter names (arch='offline', cmdm.py:63-71)
    def __init__(self, d, ff):
        super().__init__()
        self.self_attn = _MHA(d)
        self.linear1 = nn.Linear(d, ff)
        self.linear2 = nn.Linear(ff, d)
        self.norm1, self.norm2 = nn.LayerNorm(d), nn.LayerNorm(d)


class _Encoder(nn.Module):       # nn.TransformerEncoder without a final norm (the reference passes none)
    def __init__(self, d, ff, n):
        super().__init__()
        self.layers = nn.ModuleList([_EncoderLayer(d, ff) for _ in range(n)])


class _MixBlock(nn.Module):     # one block of the reference's DiffMLP (arch='mlp', model/mlp.py:9-26): parameter containers only
    def __init__(self, d, seq, first):
        super().__init__()
        self.fc0 = nn.Conv1d(seq, seq, 1)            # mixes along TIME: weight [seq, seq, 1]
        if first:
            self.conct = nn.Linear(2 * d, d)         # block 0 fuses cat(actor, reactor)
        self.emb_fc = nn.Linear(d, d)
        self.fc1 = nn.Linear(d, d)
        self.norm0, self.norm1 = nn.LayerNorm(d), nn.LayerNorm(d)


class _MixStack(nn.Module):
    def __init__(self, d, seq, n):
        super().__init__()
        self.mlps = nn.ModuleList([_MixBlock(d, seq, i == 0) for i in range(n)])


class _DiffMLP(nn.Module):      # keys mlp.motion_mlp.mlps.<l>.* (cmdm.py:85-87)
    def __init__(self, d, seq, n):
        super().__init__()
        self.motion_mlp = _MixStack(d, seq, n)


class _GRUParams(nn.Module):    # nn.GRU(d, d, num_layers)'s parameters under its names and in its order, gate order r, z, n (arch='gru', cmdm.py:84): containers only
    def __init__(self, d, n):
        super().__init__()
        for l in range(n):
            self.register_parameter(f"weight_ih_l{l}", nn.Parameter(torch.zeros(3 * d, d)))
            self.register_parameter(f"weight_hh_l{l}", nn.Parameter(torch.zeros(3 * d, d)))
            self.register_parameter(f"bias_ih_l{l}", nn.Parameter(torch.zeros(3 * d)))
            self.register_parameter(f"bias_hh_l{l}", nn.Parameter(torch.zeros(3 * d)))


class PositionalEncoding(nn.Module):
    """Sinusoid table buffer `pe` [max_len,1,d] (cmdm.py:265-276)."""

    def __init__(self, d_model, dropout=0.1, max_len=5000):
        super().__init__()
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-np.log(10000.0) / d_model))
        pe = torch.zeros(max_len, d_model)
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe.unsqueeze(1))


class TimestepEmbedder(nn.Module):
    def __init__(self, d, sequence_pos_encoder):
        super().__init__()
        self.sequence_pos_encoder = sequence_pos_encoder    # shared module -> both `pe` keys
        self.time_embed = nn.Sequential(nn.Linear(d, d), nn.SiLU(), nn.Linear(d, d))


class EmbedAction(nn.Module):
    def __init__(self, num_actions, d):
        super().__init__()
        self.action_embedding = nn.Parameter(torch.randn(num_actions, d))


class _Rot2xyzUnavailable:
    """model.rot2xyz needs a skeleton: pass CMDM(skeleton=...) or call model.set_skeleton(load_skeleton("skel.npz")) - the rest joints and
    parent table that tools/make_skeleton.py extracts from a licensed body-model file (model/rotation2xyz.py here; the reference's
    model/rotation2xyz.py:165 loads the whole SMPL-X layer instead). Or assign your own callable."""
    smpl_model = None

    def __call__(self, *a, **k):
        raise NotImplementedError(self.__doc__)


class CMDM(nn.Module):
    def __init__(self, modeltype, njoints, nfeats, num_actions, translation, pose_rep, glob, glob_rot,
                 num_frames=60, latent_dim=256, ff_size=1024, num_layers=8, num_heads=4, dropout=0.1,
                 ablation=None, activation="gelu", legacy=False, data_rep="rot6d", dataset="amass", clip_dim=512,
                 arch="trans_enc", cm_mode="add", body_model="smpl", wo_pos_emb=False, emb_trans_dec=False,
                 clip_version=None, **kargs):
        super().__init__()
        if arch not in ("online", "offline", "mlp", "gru"):
            raise NotImplementedError(
                f"arch={arch!r}: the HIP hot path runs the 'online' decoder (cmdm.py:205-227), the 'offline' encoder "
                "(cmdm.py:228-238), the 'mlp' time / feature mixer (cmdm.py:239-242) and the 'gru' stack (cmdm.py:243-249); "
                "trans_enc has no forward branch in the reference (SURVEY.md §2 row 3)")
        if arch == "gru" and cm_mode != "add":
            raise NotImplementedError(f"arch='gru' with cm_mode={cm_mode!r}: the gru branch adds the two pose embeddings and the reference "
                                      "raises NotImplementedError for anything else (cmdm.py:244-247) - pass cm_mode='add'")
        gru_scan = kargs.get("gru_scan", None) or "batch"
        if gru_scan not in _lib.GRU_SCAN:
            raise ValueError(f"gru_scan={gru_scan!r}: 'batch' (the reference's recurrence over the samples of a call) or 'frames'")
        if activation != "gelu":
            raise NotImplementedError("activation is hard-coded to gelu by the reference factory (model_util.py:70)")
        if data_rep not in ("rot6d", "xyz", "hml_vec"):
            raise ValueError(data_rep)
        if cm_mode not in ("add", "concat"):
            raise NotImplementedError(cm_mode)
        self.legacy, self.modeltype = legacy, modeltype
        self.njoints, self.nfeats, self.num_actions = njoints, nfeats, num_actions
        self.data_rep, self.dataset, self.pose_rep = data_rep, dataset, pose_rep
        self.glob, self.glob_rot, self.translation = glob, glob_rot, translation
        self.latent_dim, self.ff_size, self.num_layers, self.num_heads = latent_dim, ff_size, num_layers, num_heads
        self.dropout, self.ablation, self.activation, self.clip_dim = dropout, ablation, activation, clip_dim
        self.action_emb = kargs.get("action_emb", None)
        self.input_feats = njoints * nfeats
        self.normalize_output = kargs.get("normalize_encoder_output", False)
        self.cond_mode = kargs.get("cond_mode", "no_cond")
        self.cond_mask_prob = kargs.get("cond_mask_prob", 0.0)
        self.arch, self.cm_mode, self.num_frames = arch, cm_mode, num_frames
        self.emb_trans_dec, self.wo_pos_emb, self.body_model = emb_trans_dec, wo_pos_emb, body_model
        self.clip_version = clip_version
        # arch='gru': the axis nn.GRU scans. The reference hands [T, B, d] to a batch_first GRU, so its recurrence runs over the B samples of a call
        # ('batch', the default: what a checkpoint trained with it means); 'frames' is the recurrence over each sample's frames
        self.gru_scan = gru_scan
        if self.cond_mode not in ("no_cond", "action", "text"):
            raise NotImplementedError(f"cond_mode={self.cond_mode!r}")

        d = latent_dim
        gru_emb_dim = d if arch == "gru" else 0                      # (cmdm.py:52-54: both pose embeddings read [pose ; emb])
        self.input_process = _Pose("poseEmbedding", self.input_feats + gru_emb_dim, d)
        self.cmo_process = _Pose("poseEmbedding", self.input_feats + gru_emb_dim, d)
        self.sequence_pos_encoder = PositionalEncoding(d, dropout)
        if cm_mode == "concat":
            self.fuse_process = nn.Linear(2 * d, d)
        if arch == "offline":   # (emb_trans_dec / wo_pos_emb do not apply: the embedding is always token 0, positions always encoded)
            self.seqTransEncoder = _Encoder(d, ff_size, num_layers)
        elif arch == "gru":     # (parameter container: weight_ih_l{k} / weight_hh_l{k} / bias_ih_l{k} / bias_hh_l{k}; num_heads / ff_size are not read)
            self.gru = _GRUParams(d, num_layers)
        elif arch == "mlp":     # (no attention: num_heads / ff_size, emb_trans_dec / wo_pos_emb and cm_mode are not read; fc0 fixes the frame count)
            self.mlp = _DiffMLP(d, num_frames, num_layers)
        else:
            self.seqTransDecoder = _Decoder(d, ff_size, num_layers)
        self.embed_timestep = TimestepEmbedder(d, self.sequence_pos_encoder)
        if self.cond_mode == "text":
            self.embed_text = nn.Linear(clip_dim, d)
            # CLIP ViT-B/32 (cmdm.py:116-127) is a third-party model that is not on the hot path: supply
            # y['text_features'] [B,clip_dim] or assign `model.encode_text = callable(list[str]) -> Tensor`.
        if self.cond_mode == "action":
            self.embed_action = EmbedAction(num_actions, d)
        self.output_process = _Pose("poseFinal", d, self.input_feats)
        self.rot2xyz = _Rot2xyzUnavailable()
        if kargs.get("skeleton", None) is not None:
            self.set_skeleton(kargs["skeleton"])

        self.precision = os.environ.get("REGENNET_PRECISION", kargs.get("precision", _lib.DEFAULT_PRECISION))
        # precision schedule: split-bf16 for the last x3_tail loop indices of a sampling loop (None: engine default rule;
        # "auto": measured on this checkpoint at the first sampling call, see diffusion.calibrate_x3_tail)
        # A model that loads a checkpoint (load_state_dict) without an explicit x3_tail switches to "auto": the default rule was
        # derived from synthetic weights, so on weights nobody validated the switch point is measured (a few small runs, once).
        self.x3_tail = kargs.get("x3_tail", None)
        # ... and fp16 MFMA operands for the f16_steps plain steps in front of that tail (None: engine default 8 where the one-kernel decoder stack runs
        # the plain phase; 0: none - the default tail is then the bf16 rule's)
        self.f16_steps = kargs.get("f16_steps", None)
        # evaluations of at most this many token rows run the small-batch engine (None: engine default, 0: never)
        self.small_batch_rows = kargs.get("small_batch_rows", None)
        # evaluations of at least this many samples run the one-kernel decoder stack (k_layers; None: engine default 64, 1: always)
        self.layers_min_b = kargs.get("layers_min_b", None)
        # guided sampling on the one-kernel stack: a motion per workgroup (2) or an evaluation per workgroup and step (0); None: the engine's rule (by batch size)
        self.layers_guided = kargs.get("layers_guided", None)
        # kernel-selection switches handed to every engine this model builds (rgn_set_option: {"LAYERS": 0, "STREAMS": 1, ...}); changing the
        # dict takes effect for engines built afterwards (model._engine_stale = True rebuilds)
        self.engine_options = dict(kargs.get("engine_options", None) or {})
        self._auto_tail, self._auto_tails = None, {}
        # (multi-GPU runs: dist_util.sync_model_weights(model) synchronises THIS module's parameters once at start-up; every engine is then packed
        #  locally from them, so building one - now or later, on one rank alone - is never a collective)
        self._engine = None
        self._engines = {}
        self._engine_stale = True
        self._cond_key = None
        self._keep = None
        for p in self.parameters():
            p.requires_grad_(False)

    def set_skeleton(self, skeleton):
        """model.rot2xyz = the device forward kinematics over `skeleton` (a dict as model.rotation2xyz.load_skeleton returns it, or the path of
        such an npz); None takes it away again. Wrappers (ClassifierFreeSampleModel) follow."""
        from .rotation2xyz import Rotation2xyz, load_skeleton_or_body
        if skeleton is None:
            self.rot2xyz = _Rot2xyzUnavailable()
        else:
            self.rot2xyz = Rotation2xyz(load_skeleton_or_body(skeleton) if isinstance(skeleton, (str, os.PathLike)) else skeleton, model=self)
        return self

    # ---- nn.Module plumbing ---------------------------------------------------------------------------
    def parameters_wo_clip(self):
        return [p for name, p in self.named_parameters() if not name.startswith("clip_model.")]

    def load_state_dict(self, state_dict, strict=True):
        self._engine_stale = True
        self._auto_tail, self._auto_tails, self._warned_anchor = None, {}, False
        if self.x3_tail is None and "REGENNET_X3_TAIL" not in os.environ:
            self.x3_tail = "auto"                   # measured at the first sampling call per (schedule, sampler, guidance, T)
        return super().load_state_dict(state_dict, strict=strict)

    def _apply(self, fn, *a, **k):
        self._engine_stale = True
        return super()._apply(fn, *a, **k)

    def encode_text(self, raw_text):
        raise NotImplementedError(
            "CLIP text encoding (cmdm.py:153-166) is out of scope: pass y['text_features'] [B,clip_dim] "
            "or assign model.encode_text")

    def mask_cond(self, cond, force_mask=False):
        return torch.zeros_like(cond) if force_mask else cond   # eval-mode behaviour of cmdm.py:129-137

    def generate_square_subsequent_mask(self, sz):
        return torch.full((sz, sz), float("-inf")).triu(1)      # cmdm.py:168-171

    # ---- engine management ----------------------------------------------------------------------------
    def engine_config(self, num_frames=None):
        return dict(njoints=self.njoints, nfeats=self.nfeats, num_frames=int(num_frames or self.num_frames),
                    latent_dim=self.latent_dim, ff_size=self.ff_size, num_heads=self.num_heads, layers=self.num_layers,
                    cm_mode=self.cm_mode, cond_mode=self.cond_mode, num_actions=self.num_actions, clip_dim=self.clip_dim,
                    emb_trans_dec=self.emb_trans_dec, wo_pos_emb=self.wo_pos_emb, arch=self.arch)

    MAX_ENGINES = 16    # engines kept alive, one per sequence length (auto_regressive evaluation walks through many lengths)

    def _get_engine(self, B, T=None):
        """The engine for batches of up to B motions of T frames (default: num_frames, or the length used last). Like the
        reference's module the model itself is length-agnostic (the sequence length comes from x.shape, cmdm.py:176); an
        engine's workspace is sized per (max batch, T), so engines are cached per T (least recently used evicted) and one is
        rebuilt when a larger batch arrives."""
        if self.arch == "mlp" and T is not None and int(T) != self.num_frames:
            raise ValueError(f"arch='mlp': fc0 is Conv1d(num_frames, num_frames, 1) with num_frames = {self.num_frames} - it cannot mix {int(T)} frames")
        dev = next(self.parameters()).device
        if dev.type != "cuda" and getattr(_lib.Engine, "requires_gpu", True):
            raise RuntimeError("regennet_amd CMDM runs on an AMD GPU only: call model.to(dist_util.dev()) first "
                               "(there is no CPU fallback; the CPU restatement lives in oracle/ as a test checker)")
        if self._engine_stale:                                # weights / device changed: every cached engine is obsolete
            dist_util.synchronize(dev)
            for e in self._engines.values():
                e.close()
            self._engines.clear()
            self._engine, self._engine_stale = None, False
        T = int(T or (self._engine.cfg["num_frames"] if self._engine is not None else self.num_frames))
        eng = self._engines.pop(T, None)
        outgoing = None
        if eng is not None and (B > eng.max_batch or eng.precision != self.precision):
            dist_util.synchronize(dev)
            B = max(B, eng.max_batch)
            outgoing, eng = eng, None            # (closed once the new engine stands: a failed build leaves the cache as it was)
        if eng is None:
            while len(self._engines) >= self.MAX_ENGINES:
                dist_util.synchronize(dev)
                self._engines.pop(next(iter(self._engines))).close()
            try:
                eng = _lib.Engine(self.engine_config(T), B, dev.index or 0, self.precision, **({"options": self.engine_options} if self.engine_options else {}))
                for k, v in self.state_dict().items():
                    if k.startswith("clip_model."):
                        continue
                    eng.load_weight(k, v.detach().float().cpu().numpy())
                eng.finalize()
            except BaseException:
                # (out of memory, a refused checkpoint ...): nothing may leak, and the engine this one was to replace goes back into the cache
                if eng is not None:
                    eng.close()
                if outgoing is not None:
                    self._engines[T] = outgoing
                raise
            if outgoing is not None:
                outgoing.close()
        self._engines[T] = eng                                # (re)inserted last = most recently used
        if eng is not self._engine:
            self._engine, self._cond_key, self._keep = eng, None, None
        tail = os.environ.get("REGENNET_X3_TAIL", self.x3_tail)
        if tail == "auto":                                    # filled in per (schedule, sampler, guidance, T) by calibrate_x3_tail
            tail = self._auto_tail
        eng.set_x3_tail(-1 if tail is None else int(tail))
        eng.set_f16_steps(-1 if self.f16_steps is None else int(self.f16_steps))
        eng.set_small_batch_rows(-1 if self.small_batch_rows is None else int(self.small_batch_rows))
        eng.set_layers_min_b(-1 if self.layers_min_b is None else int(self.layers_min_b))
        if self.arch == "gru":
            eng.set_gru_scan(self.gru_scan)
        if self.arch not in ("mlp", "gru"):                   # (these engines have no k_layers and refuse its switches)
            eng.set_option("LAYERS_GUIDED", -1 if self.layers_guided is None else int(self.layers_guided))
        return eng, dev

    def _rgn_bind(self, B, y, device=None, guided=False, T=None, cache=False):
        """Bind model_kwargs['y'] on the engine. Returns (engine, guided, device).

        Sampling loops rebind on every call (one pack kernel + one GEMM: nothing next to the step loop). Only the per-step
        `forward()` API (cache=True) skips the bind for an unchanged y: the key is the identity and version counter of the
        caller's own tensors, and those tensors are held until the next bind so that their ids cannot be recycled."""
        T = int(T or self.num_frames)
        eng, dev = self._get_engine(B, T)
        cm = y["cmotion"]
        assert tuple(cm.shape) == (B, self.njoints, self.nfeats, T), \
            f"y['cmotion'] {tuple(cm.shape)} != {(B, self.njoints, self.nfeats, T)}"
        action = text = scale = None
        if self.cond_mode == "action":
            action = y["action"]
        if self.cond_mode == "text":
            text = y.get("text_features", None)
            if text is None:
                text = self.encode_text(y["text"])
        if guided:
            scale = y["scale"]
        src = (cm, action, text, scale)
        key = tuple((id(t), t._version, tuple(t.shape)) if t is not None else None for t in src) + (B, T, guided)
        if cache and key == self._cond_key:
            return eng, guided, dev
        cm_d = cm.to(device=dev, dtype=torch.float32).contiguous()
        if action is not None:
            # EmbedAction indexes a [num_actions, d] table (cmdm.py:363-365): validated on the host copy when there is one,
            # otherwise with ONE blocking read (the per-step API caches the bind, so not per step)
            a0 = action.reshape(B, -1)[:, 0]
            if bool(((a0 < 0) | (a0 >= self.num_actions)).any()):
                raise IndexError(f"y['action'] holds ids in [{int(a0.min())}, {int(a0.max())}] but the model has {self.num_actions} actions")
            action_d = a0.to(device=dev, dtype=torch.int64).contiguous()
        else:
            action_d = None
        text_d = scale_d = None
        if text is not None:
            text_d = text.to(device=dev, dtype=torch.float32).contiguous()
            assert tuple(text_d.shape) == (B, self.clip_dim)
        if scale is not None:
            scale_d = scale.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            assert tuple(scale_d.shape) == (B,)
        eng.set_condition(B, cm_d, action_d, text_d, scale_d, dist_util.stream_handle(dev))
        # device copies stay alive until the stream consumed them; the caller's tensors until the key is replaced
        self._keep = (cm_d, action_d, text_d, scale_d) + (src if cache else ())
        self._cond_key = key if cache else None
        return eng, guided, dev

    # ---- cmdm.py:173-252 -------------------------------------------------------------------------------
    def forward(self, x, timesteps, y=None, _guided=False):
        """x [B,njoints,nfeats,T] (x_t); timesteps [B] int; y dict with 'cmotion' (+ 'action'/'text_features',
        'uncond', 'scale'). Returns x0_hat [B,njoints,nfeats,T] on x's device."""
        bs, njoints, nfeats, nframes = x.shape
        assert (njoints, nfeats) == (self.njoints, self.nfeats)
        eng, _, dev = self._rgn_bind(bs, y, guided=_guided, T=nframes, cache=True)
        assert tuple(timesteps.shape) == (bs,)
        if timesteps.numel() and bool(((timesteps < 0) | (timesteps >= self.sequence_pos_encoder.pe.shape[0])).any()):
            raise IndexError("timesteps outside the positional table (TimestepEmbedder, cmdm.py:298)")
        xc = x.to(device=dev, dtype=torch.float32).contiguous()
        tc = timesteps.to(device=dev, dtype=torch.int64).contiguous()
        out = torch.empty_like(xc)
        flags = (_lib.FLAG_GUIDED if _guided else 0) | (_lib.FLAG_UNCOND if y.get("uncond", False) else 0)
        eng.denoise(xc, tc, flags, out, dist_util.stream_handle(dev))
        return out
