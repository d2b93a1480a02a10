"""Frames from meshes on the device: the counterpart of the reference's render/renderer.py (pyrender on OSMesa, one scene rebuild per frame)
and of render_video's centring and crop (render/crendermotion.py:20-42), over `rgn_render` (include/regennet_hip.h holds the contract: the
reference's camera, centring, colours, light positions and background; a Lambert model in place of its PBR material; no |Z| <= 1 clipping)."""
import numpy as np
import torch

from .. import _lib

DEFAULT_CAM = (0.75, 0.75, 0.0, 0.10)                    # crendermotion.py:20
DEFAULT_COLOR = (0.11, 0.53, 0.8)                        # crendermotion.py:20
CMDM_COLOR_2 = (0.618, 0.618, 0.618)                     # renderer.py:86-87
WHITE = (1.0, 1.0, 1.0)                                  # renderer.py:155


def default_colors(num_person, setting="cmdm", color=DEFAULT_COLOR):
    """renderer.py:86-89, 116-127: person 0 takes `color`; the others take it too under 'mdm' and the grey under 'cmdm'."""
    return [tuple(color)] + [CMDM_COLOR_2 if setting == "cmdm" else tuple(color)] * (max(1, int(num_person)) - 1)


class MeshRenderer:
    """render() for meshes of one topology: `faces` [F, 3], shared by all persons. The handle is made at the first call, when the vertex count is
    known; the workspace is the renderer's own and grows to the largest motion it has seen."""

    def __init__(self, faces, device):
        self.faces = np.ascontiguousarray(np.asarray(faces), dtype=np.int32).reshape(-1, 3)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("MeshRenderer runs on the GPU (no CPU fallback)")
        self._engine, self._work = None, None

    def close(self):
        if self._engine is not None:
            self._engine.close()
        self._engine, self._work = None, None

    def _get_engine(self, V):
        if self._engine is None or self._engine.V != V:
            self.close()
            index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self._engine = _lib.RenderEngine(self.faces, V, index)
        return self._engine

    def render(self, vertices, mask=None, width=1024, height=1024, cam=DEFAULT_CAM, colors=None, background=WHITE, center=True,
               return_buffers=False, setting="cmdm"):
        """vertices fp32 [B, V, 3 P, T] (what model.rot2xyz(..., jointstype='vertices') returns), mask bool [B, T] or None -> rgb uint8
        [B, T, H, W, 3] on the device; with return_buffers also depth fp32 [B, T, H, W] (+inf on background) and face int32 [B, T, H, W]
        (person * F + face, -1 on background). One launch sequence per motion, so the workspace stays that of one motion."""
        vertices = vertices.to(self.device, torch.float32).contiguous()
        B, V, C3, T = vertices.shape
        assert C3 % 3 == 0 and C3 >= 3, f"vertices {tuple(vertices.shape)}: channels must be 3 x num_person"
        P = C3 // 3
        if mask is not None:
            mask = mask.to(self.device).reshape(B, T).to(torch.uint8).contiguous()
        eng = self._get_engine(V)
        params = eng.params(width, height, cam, center, default_colors(P, setting) if colors is None else colors, background)
        need = eng.workspace_bytes(1, T, P, width, height)
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        rgb = torch.empty((B, T, height, width, 3), dtype=torch.uint8, device=self.device)
        depth = torch.empty((B, T, height, width), dtype=torch.float32, device=self.device) if return_buffers else None
        face = torch.empty((B, T, height, width), dtype=torch.int32, device=self.device) if return_buffers else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for b in range(B):
            eng.render(vertices[b:b + 1], None if mask is None else mask[b:b + 1], P, params, rgb[b:b + 1],
                       None if depth is None else depth[b:b + 1], None if face is None else face[b:b + 1], self._work, stream)
        return (rgb, depth, face) if return_buffers else rgb


def crop_to_content(frames, background=WHITE):
    """The box render_video crops a motion's video to (crendermotion.py:33-41): the union, over the frames [T, H, W, 3], of the pixels that are
    not background, as (y1, x1, y2, x2) with frames[:, y1:y2, x1:x2] holding all of them (the reference's slice stops one short of the last row
    and column and calls everything brighter than 0.96 background; here the background is the colour that was asked for). None when every pixel
    is background."""
    bg = [int(np.clip(np.rint(255.0 * c), 0, 255)) for c in background]
    if isinstance(frames, torch.Tensor):
        fg = (frames != torch.tensor(bg, dtype=frames.dtype, device=frames.device)).any(-1).any(0)
        rows, cols = torch.nonzero(fg.any(1)).flatten().cpu().numpy(), torch.nonzero(fg.any(0)).flatten().cpu().numpy()
    else:
        fg = (np.asarray(frames) != np.asarray(bg, dtype=np.asarray(frames).dtype)).any(-1).any(0)
        rows, cols = np.flatnonzero(fg.any(1)), np.flatnonzero(fg.any(0))
    if len(rows) == 0:
        return None
    return int(rows[0]), int(cols[0]), int(rows[-1]) + 1, int(cols[-1]) + 1
