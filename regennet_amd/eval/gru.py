"""GRU action classifier of the action2motion evaluation - host-side mirror of the reference's `eval/a2m/action2motion/models.py`
(MotionDiscriminator :6-38, MotionDiscriminatorForFID :41-61, load_classifier / load_classifier_for_fid :67-80).

Like `regennet_amd.eval.stgcn.STGCN`, the modules are checkpoint containers with the reference's parameter names and shapes
(`load_state_dict(torch.load(path)["model"])` of a reference checkpoint works unchanged); `forward` hands the motions to libregennet_hip.so
(`rgn_gru_forward`), where the frame loop, the select of each sequence's last valid frame and the two-layer head run as ONE HIP launch in fp32
arithmetic. There is no CPU fallback. The input is read as it lies ([bs, njoints, nfeats, T], frames innermost): the reference's permute to
[T, bs, features] (models.py:23-24) is never materialised.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _lib

LIN1_SIZE = 30            # models.py:16


class MotionDiscriminator(nn.Module):
    def __init__(self, input_size, hidden_size, hidden_layer, device, output_size=12, use_noise=None):
        super().__init__()
        self.device = device
        self.input_size, self.hidden_size, self.hidden_layer, self.use_noise = input_size, hidden_size, hidden_layer, use_noise
        self.output_size = output_size
        self.recurrent = nn.GRU(input_size, hidden_size, hidden_layer)
        self.linear1 = nn.Linear(hidden_size, LIN1_SIZE)
        self.linear2 = nn.Linear(LIN1_SIZE, output_size)
        self._engine, self._stale = None, True
        for p in self.parameters():
            p.requires_grad_(False)

    def load_state_dict(self, state_dict, strict=True):
        self._stale = True
        return super().load_state_dict(state_dict, strict=strict)

    def _apply(self, fn, *a, **k):
        self._stale = True
        return super()._apply(fn, *a, **k)

    def initHidden(self, num_samples, layer):
        """models.py:40-41"""
        return torch.randn(layer, num_samples, self.hidden_size, device=self.linear1.weight.device, requires_grad=False)

    def _get_engine(self):
        dev = self.linear1.weight.device
        if dev.type != "cuda":
            raise RuntimeError("regennet_amd MotionDiscriminator runs on an AMD GPU only: call model.to(device) first (no CPU fallback)")
        if self._engine is None or self._stale:
            if self._engine is not None:
                torch.cuda.synchronize(dev)
                self._engine.close()
            eng = _lib.GruEngine(self.input_size, self.hidden_size, self.hidden_layer, LIN1_SIZE, self.output_size, dev.index or 0)
            for k, v in self.state_dict().items():
                eng.load_weight(k, v.detach().float().cpu().numpy())
            eng.finalize()
            self._engine, self._stale = eng, False
        return self._engine, dev

    def forward_both(self, motion_sequence, lengths=None, hidden_unit=None, want_features=True, want_logits=True):
        """(features [bs, 30], logits [bs, output_size]) of models.py:45-61 / :20-38 from one launch; an output that is not wanted is None.
        lengths=None means every frame (the reference would fail on it). A host `lengths` tensor is checked here; one on the device is read by the
        kernel alone, which clamps a length outside [1, T] and flags it (`lengths_clamped()`), without a host synchronisation."""
        bs, njoints, nfeats, T = motion_sequence.shape
        if njoints * nfeats != self.input_size:
            raise ValueError(f"motion_sequence {tuple(motion_sequence.shape)} has {njoints * nfeats} features per frame, the classifier takes {self.input_size}")
        eng, dev = self._get_engine()
        x = motion_sequence.to(device=dev, dtype=torch.float32).contiguous()
        if lengths is None:
            lengths = torch.full((bs,), T, dtype=torch.int64)
        lengths = torch.as_tensor(lengths)
        if lengths.shape != (bs,):
            raise ValueError(f"lengths {tuple(lengths.shape)} does not match the batch of {bs}")
        if lengths.device.type == "cpu" and bs and (int(lengths.min()) < 1 or int(lengths.max()) > T):
            raise ValueError(f"lengths must lie in [1, {T}]")
        ln = lengths.to(device=dev, dtype=torch.int64).contiguous()
        if hidden_unit is None:
            hidden_unit = self.initHidden(bs, self.hidden_layer)
        if tuple(hidden_unit.shape) != (self.hidden_layer, bs, self.hidden_size):
            raise ValueError(f"hidden_unit {tuple(hidden_unit.shape)} is not [{self.hidden_layer}, {bs}, {self.hidden_size}]")
        h0 = hidden_unit.to(device=dev, dtype=torch.float32).contiguous()
        feats = torch.empty(bs, LIN1_SIZE, device=dev) if want_features else None
        logits = torch.empty(bs, self.output_size, device=dev) if want_logits else None
        eng.forward(bs, T, x, ln, h0, feats, logits, torch.cuda.current_stream(dev).cuda_stream)
        return feats, logits

    def lengths_clamped(self):
        """True when a forward since the last query was handed a length outside [1, T]. Synchronises the device."""
        return self._get_engine()[0].lengths_clamped()

    def forward(self, motion_sequence, lengths=None, hidden_unit=None):
        """models.py:20-38: logits [bs, output_size]."""
        return self.forward_both(motion_sequence, lengths, hidden_unit, want_features=False)[1]


class MotionDiscriminatorForFID(MotionDiscriminator):
    def forward(self, motion_sequence, lengths=None, hidden_unit=None):
        """models.py:45-61: features [bs, 30]."""
        return self.forward_both(motion_sequence, lengths, hidden_unit, want_logits=False)[0]


model_path = "./assets/actionrecognition/humanact12_gru.tar"      # models.py:64


def _load(cls, input_size_raw, num_classes, device, model_path, state_dict):
    if state_dict is None:
        state_dict = torch.load(model_path, map_location="cpu")["model"]
    state_dict = {k: torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v for k, v in state_dict.items()}
    classifier = cls(input_size_raw, 128, 2, device=device, output_size=num_classes)
    classifier.load_state_dict(state_dict)
    return classifier.to(device).eval()


def load_classifier(input_size_raw, num_classes, device, model_path=model_path, state_dict=None):
    """models.py:67-72; `state_dict=` takes weights that are already in memory (regennet_amd.synth.make_gru_state_dict) instead of a file."""
    return _load(MotionDiscriminator, input_size_raw, num_classes, device, model_path, state_dict)


def load_classifier_for_fid(input_size_raw, num_classes, device, model_path=model_path, state_dict=None):
    """models.py:75-80"""
    return _load(MotionDiscriminatorForFID, input_size_raw, num_classes, device, model_path, state_dict)
