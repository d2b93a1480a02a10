"""Text-motion co-embedding evaluator of the HumanML3D / KIT evaluation - host-side mirror of the reference's
`data_loaders/humanml/networks/modules.py` (MovementConvEncoder :79-98, TextEncoderBiGRUCo :311-350, MotionEncoderBiGRUCo :353-386) and
`data_loaders/humanml/networks/evaluator_wrapper.py` (EvaluatorMDMWrapper :121-187).

Like `regennet_amd.eval.gru.MotionDiscriminator`, the modules are checkpoint containers with the reference's constructor signatures, parameter names
and shapes (`load_state_dict(checkpoint['motion_encoder'])` of a reference `finest.tar` works unchanged); `forward` hands the tensors to
libregennet_hip.so (`rgn_t2m_*`), where the convolutions, the hoisted input products, the bidirectional recurrence and the head run as HIP kernels in
fp32 arithmetic. There is no CPU fallback. The kernels are order-free: rows need not be sorted by length, as `pack_padded_sequence` demands.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _lib

UNIT_LENGTH = 4                       # evaluator_wrapper.py:138
_NEUTRAL = dict(dim_pose=263, movement_hidden=512, movement_latent=512, motion_hidden=1024, dim_word=300, dim_pos_ohot=15, text_hidden=512, coemb=512,
                unit_length=UNIT_LENGTH)
_PREFIX = {"movement": "movement_encoder.", "text": "text_encoder.", "motion": "motion_encoder."}


def _fill(prefix, shapes, seed):
    """deterministic stand-in weights for the sub-models a stand-alone module does not own (the engine wants all three; they are never run)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return {prefix + k: (0.01 * rng.standard_normal(s)).astype(np.float32) for k, s in shapes.items()}


def _bigru_shapes(H, D):
    sh = {"hidden": (2, 1, H), "output_net.0.weight": (H, 2 * H), "output_net.0.bias": (H,), "output_net.1.weight": (H,), "output_net.1.bias": (H,),
          "output_net.3.weight": (D, H), "output_net.3.bias": (D,)}
    for s in ("_l0", "_l0_reverse"):
        sh.update({"gru.weight_ih" + s: (3 * H, H), "gru.weight_hh" + s: (3 * H, H), "gru.bias_ih" + s: (3 * H,), "gru.bias_hh" + s: (3 * H,)})
    return sh


def _shapes(geo):
    C, Hm, Dm, H, W, P, Ht, D = (geo[k] for k in ("dim_pose", "movement_hidden", "movement_latent", "motion_hidden", "dim_word", "dim_pos_ohot",
                                                   "text_hidden", "coemb"))
    C -= 4
    return {"movement": {"main.0.weight": (Hm, C, 4), "main.0.bias": (Hm,), "main.3.weight": (Dm, Hm, 4), "main.3.bias": (Dm,),
                         "out_net.weight": (Dm, Dm), "out_net.bias": (Dm,)},
            "text": dict(_bigru_shapes(Ht, D), **{"pos_emb.weight": (W, P), "pos_emb.bias": (W,), "input_emb.weight": (Ht, W), "input_emb.bias": (Ht,)}),
            "motion": dict(_bigru_shapes(H, D), **{"input_emb.weight": (H, Dm), "input_emb.bias": (H,)})}


def make_engine(geo, parts, device):
    """A finalized `_lib.T2mEngine` for the geometry: `parts` maps 'movement' / 'text' / 'motion' to a state dict; a missing part gets stand-in weights."""
    eng = _lib.T2mEngine(geo, device.index or 0)
    for part, shapes in _shapes(geo).items():
        sd = parts.get(part)
        if sd is None:
            sd = {k[len(_PREFIX[part]):]: v for k, v in _fill(_PREFIX[part], shapes, 7).items()}
        for k in shapes:
            v = sd[k]
            eng.load_weight(_PREFIX[part] + k, v.detach().float().cpu().numpy() if torch.is_tensor(v) else np.asarray(v, np.float32))
    eng.finalize()
    return eng


class _EngineModule(nn.Module):
    """What the three modules share: the engine is rebuilt when the parameters changed (load_state_dict, .to())."""
    _part = None

    def _init_engine(self):
        self._engine, self._stale, self._owner = None, True, None       # _owner: the EvaluatorMDMWrapper whose engine this module shares
        for p in self.parameters():
            p.requires_grad_(False)

    def load_state_dict(self, state_dict, strict=True):
        self._stale = True
        return super().load_state_dict(state_dict, strict=strict)

    def _apply(self, fn, *a, **k):
        self._stale = True
        return super()._apply(fn, *a, **k)

    def _geometry(self):
        raise NotImplementedError

    def _get_engine(self):
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(f"regennet_amd {type(self).__name__} runs on an AMD GPU only: call model.to(device) first (no CPU fallback)")
        if self._owner is not None and dev == self._owner.device:
            return self._owner._get_engine(), dev
        if self._engine is None or self._stale:
            if self._engine is not None:
                torch.cuda.synchronize(dev)
                self._engine.close()
            self._engine, self._stale = make_engine(self._geometry(), {self._part: self.state_dict()}, dev), False
        return self._engine, dev

    def lengths_clamped(self):
        """True when a forward since the last query was handed a length outside its range. Synchronises the device."""
        return self._get_engine()[0].lengths_clamped()


def _lens(lens, n, dev):
    lens = torch.as_tensor(lens)
    if lens.shape != (n,):
        raise ValueError(f"lengths {tuple(lens.shape)} do not match the batch of {n}")
    return lens.to(device=dev, dtype=torch.int64).contiguous()


class MovementConvEncoder(_EngineModule):
    _part = "movement"

    def __init__(self, input_size, hidden_size, output_size):
        super().__init__()
        self.main = nn.Sequential(nn.Conv1d(input_size, hidden_size, 4, 2, 1), nn.Dropout(0.2, inplace=True), nn.LeakyReLU(0.2, inplace=True),
                                  nn.Conv1d(hidden_size, output_size, 4, 2, 1), nn.Dropout(0.2, inplace=True), nn.LeakyReLU(0.2, inplace=True))
        self.out_net = nn.Linear(output_size, output_size)
        self.input_size, self.hidden_size, self.output_size = input_size, hidden_size, output_size
        self._init_engine()

    def _geometry(self):
        return dict(_NEUTRAL, dim_pose=self.input_size + 4, movement_hidden=self.hidden_size, movement_latent=self.output_size, motion_hidden=64,
                    text_hidden=64, dim_word=4, dim_pos_ohot=1, coemb=4)

    def forward(self, inputs, m_lens=None):
        """modules.py:94-98: inputs [N, T, input_size] (any frame stride: a slice motions[..., :-4] is read in place) -> [N, T2, output_size]. With
        m_lens (frames) only movement frames below m_lens // 4 are computed; the others are zero."""
        N, T, C = inputs.shape
        if C != self.input_size:
            raise ValueError(f"inputs {tuple(inputs.shape)} have {C} features per frame, the encoder takes {self.input_size}")
        eng, dev = self._get_engine()
        x = inputs.to(device=dev, dtype=torch.float32)
        if x.stride(2) != 1 or x.stride(0) != T * x.stride(1) or x.stride(1) < C:
            x = x.contiguous()
        T2 = ((T - 2) // 2 + 1 - 2) // 2 + 1
        out = torch.zeros(N, T2, self.output_size, device=dev)
        eng.movements(N, T, x.stride(1), x, None if m_lens is None else _lens(m_lens, N, dev), out, torch.cuda.current_stream(dev).cuda_stream)
        return out


class _BiGRUCo(_EngineModule):
    def _build(self, input_size, hidden_size, output_size):
        self.input_emb = nn.Linear(input_size, hidden_size)
        self.gru = nn.GRU(hidden_size, hidden_size, batch_first=True, bidirectional=True)
        self.output_net = nn.Sequential(nn.Linear(hidden_size * 2, hidden_size), nn.LayerNorm(hidden_size), nn.LeakyReLU(0.2, inplace=True),
                                        nn.Linear(hidden_size, output_size))
        self.hidden_size, self.output_size = hidden_size, output_size
        self.hidden = nn.Parameter(torch.randn((2, 1, hidden_size)))


class TextEncoderBiGRUCo(_BiGRUCo):
    _part = "text"

    def __init__(self, word_size, pos_size, hidden_size, output_size, device):
        super().__init__()
        self.device = device
        self.word_size, self.pos_size = word_size, pos_size
        self.pos_emb = nn.Linear(pos_size, word_size)
        self._build(word_size, hidden_size, output_size)
        self._init_engine()

    def _geometry(self):
        return dict(_NEUTRAL, dim_pose=5, movement_hidden=64, movement_latent=64, motion_hidden=64, dim_word=self.word_size, dim_pos_ohot=self.pos_size,
                    text_hidden=self.hidden_size, coemb=self.output_size)

    def forward(self, word_embs, pos_onehot, cap_lens):
        """modules.py:335-350: word_embs [N, Lw, word_size], pos_onehot [N, Lw, pos_size], cap_lens [N] in [1, Lw] -> [N, output_size]"""
        N, Lw, _ = word_embs.shape
        eng, dev = self._get_engine()
        out = torch.empty(N, self.output_size, device=dev)
        eng.text_embeddings(N, Lw, word_embs.to(device=dev, dtype=torch.float32).contiguous(), pos_onehot.to(device=dev, dtype=torch.float32).contiguous(),
                            _lens(cap_lens, N, dev), out, torch.cuda.current_stream(dev).cuda_stream)
        return out


class MotionEncoderBiGRUCo(_BiGRUCo):
    _part = "motion"

    def __init__(self, input_size, hidden_size, output_size, device):
        super().__init__()
        self.device = device
        self.input_size = input_size
        self._build(input_size, hidden_size, output_size)
        self._init_engine()

    def _geometry(self):
        return dict(_NEUTRAL, dim_pose=5, movement_hidden=64, movement_latent=self.input_size, motion_hidden=self.hidden_size, dim_word=4, dim_pos_ohot=1,
                    text_hidden=64, coemb=self.output_size)

    def forward(self, inputs, m_lens):
        """modules.py:373-386: inputs [N, T2, input_size] (movements), m_lens [N] in [1, T2] (movement frames) -> [N, output_size]"""
        N, T2, _ = inputs.shape
        eng, dev = self._get_engine()
        out = torch.empty(N, self.output_size, device=dev)
        eng.encode_movements(N, T2, inputs.to(device=dev, dtype=torch.float32).contiguous(), _lens(m_lens, N, dev), out,
                             torch.cuda.current_stream(dev).cuda_stream)
        return out


def build_evaluators(opt, checkpoint=None, state_dicts=None):
    """evaluator_wrapper.py:95-118. `state_dicts` takes weights that are already in memory ({'movement_encoder', 'text_encoder', 'motion_encoder'},
    e.g. regennet_amd.synth.make_t2m_state_dicts) instead of a file."""
    movement_enc = MovementConvEncoder(opt["dim_pose"] - 4, opt["dim_movement_enc_hidden"], opt["dim_movement_latent"])
    text_enc = TextEncoderBiGRUCo(word_size=opt["dim_word"], pos_size=opt["dim_pos_ohot"], hidden_size=opt["dim_text_hidden"],
                                  output_size=opt["dim_coemb_hidden"], device=opt["device"])
    motion_enc = MotionEncoderBiGRUCo(input_size=opt["dim_movement_latent"], hidden_size=opt["dim_motion_hidden"], output_size=opt["dim_coemb_hidden"],
                                      device=opt["device"])
    if state_dicts is None:
        state_dicts = torch.load(checkpoint, map_location="cpu")
        print("Loading Evaluation Model Wrapper (Epoch %d) Completed!!" % (state_dicts["epoch"]))
    for module, key in ((movement_enc, "movement_encoder"), (text_enc, "text_encoder"), (motion_enc, "motion_encoder")):
        module.load_state_dict({k: v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v)) for k, v in state_dicts[key].items()})
    return text_enc, motion_enc, movement_enc


class EvaluatorMDMWrapper(object):
    """evaluator_wrapper.py:121-187. One engine serves the three modules; the embeddings come back as device tensors in the reference's row order
    (motions sorted by length, longest first; text rows reordered alike) unless keep_order=True asks for the input order."""

    def __init__(self, dataset_name, device, checkpoint=None, state_dicts=None, **geometry):
        opt = {"dataset_name": dataset_name, "device": device, "dim_word": 300, "max_motion_length": 196, "dim_pos_ohot": 15, "dim_motion_hidden": 1024,
               "max_text_len": 20, "dim_text_hidden": 512, "dim_coemb_hidden": 512, "dim_pose": 263 if dataset_name == "humanml" else 251,
               "dim_movement_enc_hidden": 512, "dim_movement_latent": 512, "checkpoints_dir": ".", "unit_length": UNIT_LENGTH}
        opt.update(geometry)                                   # (tests run reduced geometries)
        if checkpoint is None and state_dicts is None:
            ckpt_dir = "t2m" if dataset_name == "humanml" else dataset_name
            checkpoint = f"./{ckpt_dir}/text_mot_match/model/finest.tar"
        self.text_encoder, self.motion_encoder, self.movement_encoder = build_evaluators(opt, checkpoint, state_dicts)
        self.opt = opt
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", 0)
        for m in (self.text_encoder, self.motion_encoder, self.movement_encoder):
            m.to(self.device).eval()
            m._owner = self                                    # called on their own, the sub-modules run on the wrapper's engine
        self._engine = None

    def geometry(self):
        o = self.opt
        return dict(dim_pose=o["dim_pose"], movement_hidden=o["dim_movement_enc_hidden"], movement_latent=o["dim_movement_latent"],
                    motion_hidden=o["dim_motion_hidden"], dim_word=o["dim_word"], dim_pos_ohot=o["dim_pos_ohot"], text_hidden=o["dim_text_hidden"],
                    coemb=o["dim_coemb_hidden"], unit_length=o["unit_length"])

    def _get_engine(self):
        if self.device.type != "cuda":
            raise RuntimeError("regennet_amd EvaluatorMDMWrapper runs on an AMD GPU only (no CPU fallback)")
        mods = (self.text_encoder, self.motion_encoder, self.movement_encoder)
        if self._engine is not None and any(m._stale for m in mods):     # a sub-module's weights changed since the engine was built
            torch.cuda.synchronize(self.device)
            self._engine.close()
            self._engine = None
        if self._engine is None:
            for m in mods:
                m._stale = False
            self._engine = make_engine(self.geometry(), {"movement": self.movement_encoder.state_dict(), "text": self.text_encoder.state_dict(),
                                                         "motion": self.motion_encoder.state_dict()}, self.device)
        return self._engine

    def lengths_clamped(self):
        return self._get_engine().lengths_clamped()

    @staticmethod
    def align_idx(m_lens):
        """evaluator_wrapper.py:160"""
        return np.argsort(torch.as_tensor(m_lens).tolist())[::-1].copy()

    def _motion(self, motions, m_lens):
        eng, dev = self._get_engine(), self.device
        motions = motions.detach().to(device=dev, dtype=torch.float32).contiguous()
        N, T, C = motions.shape
        if C != self.opt["dim_pose"]:
            raise ValueError(f"motions {tuple(motions.shape)} have {C} features per frame, the evaluator takes {self.opt['dim_pose']}")
        out = torch.empty(N, self.opt["dim_coemb_hidden"], device=dev)
        eng.motion_embeddings(N, T, motions, _lens(m_lens, N, dev), out, torch.cuda.current_stream(dev).cuda_stream)
        return out

    def get_co_embeddings(self, word_embs, pos_ohot, cap_lens, motions, m_lens, keep_order=False):
        """evaluator_wrapper.py:154-172 -> (text_embedding, motion_embedding), device tensors [N, 512]"""
        with torch.no_grad():
            eng, dev = self._get_engine(), self.device
            N, Lw, _ = word_embs.shape
            text = torch.empty(N, self.opt["dim_coemb_hidden"], device=dev)
            eng.text_embeddings(N, Lw, word_embs.detach().to(device=dev, dtype=torch.float32).contiguous(),
                                pos_ohot.detach().to(device=dev, dtype=torch.float32).contiguous(), _lens(cap_lens, N, dev), text,
                                torch.cuda.current_stream(dev).cuda_stream)
            motion = self._motion(motions, m_lens)
            if not keep_order:
                idx = torch.from_numpy(self.align_idx(m_lens)).to(dev)
                text, motion = text[idx], motion[idx]
        return text, motion

    def get_motion_embeddings(self, motions, m_lens, keep_order=False):
        """evaluator_wrapper.py:175-187"""
        with torch.no_grad():
            motion = self._motion(motions, m_lens)
            if not keep_order:
                motion = motion[torch.from_numpy(self.align_idx(m_lens)).to(self.device)]
        return motion
