"""ctypes binding of libregennet_hip.so (C-ABI: include/regennet_hip.h).

The product path has NO CPU fallback: if the HIP library has not been built
(`python -c "import __graft_entry__ as g; g.build()"`) importing this module raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libregennet_hip.so")

RGN_OK = 0
RGN_ERR_UNSUPPORTED = -7
ERR_NAMES = {-1: "INVALID_ARG", -2: "BAD_KEY", -3: "BAD_SHAPE", -4: "MISSING_KEY", -5: "STATE", -6: "HIP", -7: "UNSUPPORTED", -8: "INTERNAL"}
CM = {"add": 0, "concat": 1}
ARCH = {"online": 0, "offline": 1, "mlp": 3, "gru": 4}     # RGN_ARCH_* (include/regennet_hip.h)
GRU_SCAN = {"batch": 0, "frames": 1}              # RGN_GRU_SCAN_*: the axis an arch='gru' model scans
COND = {"no_cond": 0, "action": 1, "text": 2}
PREC = {"f32": 0, "bf16x3": 1, "bf16": 2, "bf16_x3tail": 3}
DEFAULT_PRECISION = "bf16_x3tail"
SAMPLER = {"ddpm": 0, "ddim": 1}
FLAG_UNCOND, FLAG_GUIDED = 1, 2
POSE_REP = {"rot6d": 0, "rotvec": 1, "rotquat": 2, "rotmat": 3}     # RGN_POSE_*; channels per rotation below
POSE_REP_CHANNELS = {"rot6d": 6, "rotvec": 3, "rotquat": 4, "rotmat": 9}
R2X_TRANSLATION, R2X_GLOB, R2X_VERTSTRANS = 1, 2, 4
LOSS_FC = 1                                                          # RGN_LOSS_FC
LOSS_TERMS = ("rot_mse", "rcxyz_mse", "vel_mse", "fc", "orient", "body", "transl")      # the columns of rgn_loss_terms (RGN_LOSS_*)
VB_CLIP = 1                                                          # RGN_VB_CLIP
VB_TERMS = ("vb", "xstart_mse", "mse")                               # the columns of rgn_vb_terms (RGN_VB_*)


class RgnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"regennet_hip error {code} ({ERR_NAMES.get(code, '?')}): {msg}")
        self.code = code


class RgnConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "njoints", "nfeats", "num_frames", "latent_dim", "ff_size", "num_heads", "num_layers", "cm_mode",
        "cond_mode", "num_actions", "clip_dim", "emb_trans_dec", "wo_pos_emb", "max_batch", "precision", "device", "arch")]


class RgnSchedule(C.Structure):
    _fields_ = [("S", C.c_int32), ("timestep_map", C.POINTER(C.c_int64))] + [
        (n, C.POINTER(C.c_double)) for n in (
            "posterior_mean_coef1", "posterior_mean_coef2", "model_log_variance", "sqrt_recip_alphas_cumprod",
            "sqrt_recipm1_alphas_cumprod", "alphas_cumprod", "alphas_cumprod_prev")]


# every symbol include/regennet_hip.h declares: name -> (restype, argtypes)
_vp, _i32, _i64, _u64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float
SYMBOLS = {
    "rgn_create": (C.c_int, [C.POINTER(RgnConfig), C.POINTER(_vp)]),
    "rgn_destroy": (C.c_int, [_vp]),
    "rgn_last_error": (C.c_char_p, [_vp]),
    "rgn_load_weight": (C.c_int, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i32]),
    "rgn_finalize_weights": (C.c_int, [_vp]),
    "rgn_weight_blob": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    "rgn_set_schedule": (C.c_int, [_vp, C.POINTER(RgnSchedule)]),
    "rgn_set_condition": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "rgn_denoise": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp]),
    "rgn_sample_range": (C.c_int, [_vp, _i32, _i32, _f32, _vp, _vp, _u64, _u64, _i32, _i32, _vp, _i32, _i32, _vp]),
    "rgn_set_x3_tail": (C.c_int, [_vp, _i32]),
    "rgn_set_f16_steps": (C.c_int, [_vp, _i32]),
    "rgn_precision_plan": (C.c_int, [_vp, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "rgn_set_small_batch_rows": (C.c_int, [_vp, _i32]),
    "rgn_set_const_noise": (C.c_int, [_vp, _i32]),
    "rgn_set_inpainting": (C.c_int, [_vp, _i32, _vp, _vp, _vp]),
    "rgn_set_option": (C.c_int, [_vp, C.c_char_p, _i32]),
    "rgn_set_layers_min_b": (C.c_int, [_vp, _i32]),
    "rgn_set_gru_scan": (C.c_int, [_vp, _i32]),
    "rgn_gru_stack_info": (C.c_int, [_vp, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_u64)]),
    "rgn_plan_query": (C.c_int, [_vp, _i32, _i32, _i32, _i32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rgn_randn": (C.c_int, [_vp, _vp, _i32, _u64, _u64, _vp]),
    "rgn_randn_step": (C.c_int, [_vp, _vp, _i32, _u64, _u64, _i32, _vp]),
    "rgn_rot6d_to_matrix": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "rgn_gaussian_filter1d": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _f32, _vp]),
    "rgn_rot2xyz": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "rgn_rot2xyz_shaped": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "rgn_loss_terms": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _f32, _i32, _vp, _vp]),
    "rgn_q_sample_rows": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _u64, _u64, _vp, _vp, _vp]),
    "rgn_vb_terms": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "rgn_hml_to_joints": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "rgn_profile_enable": (C.c_int, [_vp, _i32]),
    "rgn_profile_query": (C.c_int, [_vp, _i32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(_i64)]),
    "rgn_profile_bracket_overhead": (C.c_int, [_vp, C.POINTER(C.c_double)]),
}

class RgnStgcnConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("in_channels", "num_class", "num_person", "num_nodes", "num_frames", "max_batch", "device")]


SYMBOLS.update({
    "rgn_stgcn_create": (C.c_int, [C.POINTER(RgnStgcnConfig), C.POINTER(_vp)]),
    "rgn_stgcn_destroy": (C.c_int, [_vp]),
    "rgn_stgcn_last_error": (C.c_char_p, [_vp]),
    "rgn_stgcn_load_weight": (C.c_int, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i32]),
    "rgn_stgcn_set_blocks": (C.c_int, [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "rgn_stgcn_check_blocks": (C.c_int, [_i32, C.POINTER(_i32), C.POINTER(_i32), C.c_char_p, _i32]),
    "rgn_stgcn_finalize": (C.c_int, [_vp]),
    "rgn_stgcn_set_option": (C.c_int, [_vp, C.c_char_p, _i32]),
    "rgn_stgcn_forward": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp]),
})

SYMBOLS.update({
    "rgn_body_create": (C.c_int, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, C.POINTER(_vp)]),
    "rgn_body_destroy": (C.c_int, [_vp]),
    "rgn_body_last_error": (C.c_char_p, [_vp]),
    "rgn_rot2verts_workspace": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(_u64)]),
    "rgn_rot2verts": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "rgn_rot2verts_shaped_workspace": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(_u64)]),
    "rgn_rot2verts_shaped": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _u64,
                                       _vp]),
    "rgn_body_set_joint_regressors": (C.c_int, [_vp, _i32, _vp, _i32, _vp]),
    "rgn_rot2joints_workspace": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(_u64)]),
    "rgn_rot2joints": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _u64, _vp]),
    "rgn_rot2joints_shaped_workspace": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(_u64)]),
    "rgn_rot2joints_shaped": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp,
                                        _vp, _vp, _u64, _vp]),
})

RENDER_MAX_PERSONS = 8                 # RGN_RENDER_MAX_PERSONS


class RgnRenderParams(C.Structure):
    _fields_ = [("width", _i32), ("height", _i32), ("cam", _f32 * 4), ("center", _i32), ("colors", (_f32 * 3) * RENDER_MAX_PERSONS), ("background", _f32 * 3)]


SYMBOLS.update({
    "rgn_render_create": (C.c_int, [_i32, _i32, _i32, _vp, C.POINTER(_vp)]),
    "rgn_render_destroy": (C.c_int, [_vp]),
    "rgn_render_last_error": (C.c_char_p, [_vp]),
    "rgn_render_workspace": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(_u64)]),
    "rgn_render": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, C.POINTER(RgnRenderParams), _vp, _vp, _vp, _vp, _u64, _vp]),
})

# the metrics of the unconstrained evaluation (rgn_metrics.hip): no handle, errors through rgn_last_error(NULL)
SYMBOLS.update({
    "rgn_poly_mmd_workspace": (C.c_int, [_i32, _i32, C.POINTER(_u64)]),
    "rgn_poly_mmd": (C.c_int, [_i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _u64, _vp]),
    "rgn_knn_radius": (C.c_int, [_i32, _vp, _i32, _i32, _i32, _vp, _vp]),
    "rgn_manifold_hits": (C.c_int, [_i32, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
})


class RgnGruConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("input_size", "hidden_size", "num_layers", "lin1_size", "output_size", "device")]


# the GRU action classifier of the action2motion evaluation (rgn_gru.hip)
SYMBOLS.update({
    "rgn_gru_create": (C.c_int, [C.POINTER(RgnGruConfig), C.POINTER(_vp)]),
    "rgn_gru_destroy": (C.c_int, [_vp]),
    "rgn_gru_last_error": (C.c_char_p, [_vp]),
    "rgn_gru_load_weight": (C.c_int, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i32]),
    "rgn_gru_finalize": (C.c_int, [_vp]),
    "rgn_gru_forward": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rgn_gru_length_status": (C.c_int, [_vp, C.POINTER(_i32)]),
})



class RgnT2mConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("device", "dim_pose", "movement_hidden", "movement_latent", "motion_hidden", "dim_word", "dim_pos_ohot",
                                         "text_hidden", "coemb", "unit_length")]


# the text-to-motion evaluation: movement encoder, bi-GRU co-embedding encoders, matching (rgn_t2m.hip)
SYMBOLS.update({
    "rgn_t2m_create": (C.c_int, [C.POINTER(RgnT2mConfig), C.POINTER(_vp)]),
    "rgn_t2m_destroy": (C.c_int, [_vp]),
    "rgn_t2m_last_error": (C.c_char_p, [_vp]),
    "rgn_t2m_load_weight": (C.c_int, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i32]),
    "rgn_t2m_finalize": (C.c_int, [_vp]),
    "rgn_t2m_workspace": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(C.c_size_t)]),
    "rgn_t2m_movements": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "rgn_t2m_encode_movements": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "rgn_t2m_motion_embeddings": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "rgn_t2m_text_embeddings": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "rgn_t2m_length_status": (C.c_int, [_vp, C.POINTER(_i32)]),
    "rgn_t2m_match": (C.c_int, [_i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
})

_lib = None


def default_x3_tail(S, layers=8, etd=False):
    """The engine's default split-bf16 tail where the plain phase has NO fp16 sub-phase (rgn_plan.cpp default_tail(): kernel-per-stage forms,
    150-frame models, batches below 64, "BULK_F16": 0): how many of the last loop indices run split-bf16. Host-side mirror for tests; what an
    engine will actually do for a batch on its bound schedule is Engine.precision_plan()."""
    if etd:
        return S
    if layers >= 8:
        if S <= 10:
            return min(S, 3)
        return min(S, max(5, -(-S // 200)))
    return min(S, -(-max(8, -(-S // 100)) * 8 // max(1, layers)))


def load():
    """Load the shared library (once) and type every entry point. Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` from the repo root.")
    # PyTorch-ROCm bundles its own libamdhip64 (SONAME libamdhip64.so.7). It must be in the process BEFORE
    # our library so that both bind to ONE HIP runtime (streams/events/pointers are shared with torch).
    import torch  # noqa: F401
    rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(rt):
        C.CDLL(rt, mode=C.RTLD_GLOBAL)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)      # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Engine:
    """Owns one rgn_handle. Thin, typed wrappers; tensors are torch CUDA(HIP) tensors, fp32/int64 contiguous."""

    def __init__(self, cfg, max_batch, device_index, precision="f32", options=None):
        """options: {switch: int} for rgn_set_option - the REGENNET_<KEY> kernel-selection switches for THIS engine only."""
        self.lib = load()
        self.cfg = dict(cfg)
        self.max_batch = int(max_batch)
        self.precision = precision
        rc = RgnConfig(
            njoints=cfg["njoints"], nfeats=cfg["nfeats"], num_frames=cfg["num_frames"], latent_dim=cfg["latent_dim"],
            ff_size=cfg["ff_size"], num_heads=cfg["num_heads"], num_layers=cfg["layers"], cm_mode=CM[cfg["cm_mode"]],
            cond_mode=COND[cfg["cond_mode"]], num_actions=int(cfg.get("num_actions", 1)), clip_dim=int(cfg.get("clip_dim", 512)),
            emb_trans_dec=int(bool(cfg.get("emb_trans_dec", False))), wo_pos_emb=int(bool(cfg.get("wo_pos_emb", False))),
            max_batch=self.max_batch, precision=PREC[precision], device=int(device_index), arch=ARCH[cfg.get("arch", "online")])
        h = C.c_void_p()
        code = self.lib.rgn_create(C.byref(rc), C.byref(h))
        if code != RGN_OK:
            raise RgnError(code, (self.lib.rgn_last_error(None) or b"").decode())
        self.h = h
        self.schedule_id = None
        self.cond_key = None
        for k, v in (options or {}).items():
            self._ck(self.lib.rgn_set_option(self.h, str(k).encode(), int(v)))

    def _ck(self, code):
        if code != RGN_OK:
            raise RgnError(code, (self.lib.rgn_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.rgn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights -------------------------------------------------------------------------------
    def load_weight(self, key, array):
        a = np.ascontiguousarray(array, dtype=np.float32)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        self._ck(self.lib.rgn_load_weight(self.h, key.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))

    def finalize(self):
        self._ck(self.lib.rgn_finalize_weights(self.h))

    def weight_blob(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._ck(self.lib.rgn_weight_blob(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---- schedule / condition ----------------------------------------------------------------------
    def set_schedule(self, timestep_map, tables, sched_id=None):
        keep = []

        def dptr(name):
            a = np.ascontiguousarray(tables[name], dtype=np.float64)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(C.c_double))

        tm = np.ascontiguousarray(timestep_map, dtype=np.int64)
        s = RgnSchedule(S=len(tm), timestep_map=tm.ctypes.data_as(C.POINTER(C.c_int64)),
                        posterior_mean_coef1=dptr("posterior_mean_coef1"), posterior_mean_coef2=dptr("posterior_mean_coef2"),
                        model_log_variance=dptr("model_log_variance"),
                        sqrt_recip_alphas_cumprod=dptr("sqrt_recip_alphas_cumprod"),
                        sqrt_recipm1_alphas_cumprod=dptr("sqrt_recipm1_alphas_cumprod"),
                        alphas_cumprod=dptr("alphas_cumprod"), alphas_cumprod_prev=dptr("alphas_cumprod_prev"))
        self._ck(self.lib.rgn_set_schedule(self.h, C.byref(s)))
        self.schedule_id = sched_id

    def set_condition(self, B, cmotion, action, text_feat, scale, stream):
        self._ck(self.lib.rgn_set_condition(self.h, int(B), _ptr(cmotion), _ptr(action), _ptr(text_feat), _ptr(scale),
                                            C.c_void_p(stream)))

    # ---- compute -----------------------------------------------------------------------------------
    def denoise(self, x, t, flags, out, stream):
        self._ck(self.lib.rgn_denoise(self.h, _ptr(x), _ptr(t), int(flags), _ptr(out), C.c_void_p(stream)))

    def sample_range(self, sampler, guided, eta, x, noise, seed, sample_offset, first_index, count, x0_out, use_graph,
                     clip_denoised, stream):
        self._ck(self.lib.rgn_sample_range(self.h, SAMPLER[sampler], int(bool(guided)), float(eta), _ptr(x), _ptr(noise),
                                           int(seed) & (2 ** 64 - 1), int(sample_offset), int(first_index), int(count),
                                           _ptr(x0_out), int(bool(use_graph)), int(bool(clip_denoised)), C.c_void_p(stream)))

    def set_x3_tail(self, tail_steps):
        """Precision schedule ('bf16_x3tail'): split-bf16 for the last `tail_steps` loop indices (-1: default)."""
        self._ck(self.lib.rgn_set_x3_tail(self.h, int(tail_steps)))

    def set_f16_steps(self, steps):
        """Precision schedule: the `steps` plain loop indices in front of the split-bf16 tail run on fp16 MFMA operands (-1: default 8; 0: none)."""
        self._ck(self.lib.rgn_set_f16_steps(self.h, int(steps)))

    def precision_plan(self, B, guided=False):
        """(f16_steps, x3_tail) rgn_sample_range will use for B motions on the bound schedule: loop indices < x3_tail split-bf16, the next f16_steps
        plain fp16, the rest plain bf16."""
        n16, tail = _i32(), _i32()
        self._ck(self.lib.rgn_precision_plan(self.h, int(B), int(bool(guided)), C.byref(n16), C.byref(tail)))
        return n16.value, tail.value

    def set_const_noise(self, on):
        """p_sample's const_noise (gaussian_diffusion.py:544-547) for the following sample_range calls."""
        self._ck(self.lib.rgn_set_const_noise(self.h, int(bool(on))))

    def set_inpainting(self, mask, motion, stream):
        """In-painting (gaussian_diffusion.py:319-323) for the following sample_range calls: mask bool / uint8 [B,njoints,nfeats,T],
        motion fp32 of the same shape, both contiguous on the engine's device. The engine copies them (on `stream`)."""
        assert mask.is_contiguous() and motion.is_contiguous() and mask.element_size() == 1 and motion.dtype.is_floating_point and motion.element_size() == 4
        assert tuple(mask.shape) == tuple(motion.shape)
        self._ck(self.lib.rgn_set_inpainting(self.h, int(mask.shape[0]), _ptr(mask), _ptr(motion), C.c_void_p(stream)))

    def clear_inpainting(self):
        self._ck(self.lib.rgn_set_inpainting(self.h, 0, None, None, None))

    def set_small_batch_rows(self, rows):
        """Evaluations of at most `rows` token rows run the small-batch (column-split) kernels; -1: default, 0: off."""
        self._ck(self.lib.rgn_set_small_batch_rows(self.h, int(rows)))

    def set_option(self, key, value):
        """rgn_set_option on the live handle: before finalize any switch; afterwards only the dispatch rules that may change between calls
        ("LAYERS_GUIDED": 0 an evaluation per workgroup | 1 by batch size | 2 a motion per workgroup | -1 the engine's default)."""
        self._ck(self.lib.rgn_set_option(self.h, str(key).encode(), int(value)))

    def set_layers_min_b(self, samples):
        """Evaluations of at least `samples` samples (<= 64 tokens) run the one-kernel decoder stack (k_layers); -1: default (64)."""
        self._ck(self.lib.rgn_set_layers_min_b(self.h, int(samples)))

    def set_gru_scan(self, scan):
        """arch='gru' engines: the axis the GRU scans, 'batch' (the reference's: sample b depends on samples 0 .. b - 1 of the call) or 'frames'."""
        self._ck(self.lib.rgn_set_gru_scan(self.h, GRU_SCAN[scan] if isinstance(scan, str) else int(scan)))

    def gru_stack_info(self, B, guided=False):
        """arch='gru' engines: dict(scan, segments, steps, launches_per_eval, workspace_bytes) of the stack for an evaluation of B motions."""
        scan, seg, steps, n, ws = _i32(), _i32(), _i32(), _i32(), _u64()
        self._ck(self.lib.rgn_gru_stack_info(self.h, int(B), int(bool(guided)), C.byref(scan), C.byref(seg), C.byref(steps), C.byref(n), C.byref(ws)))
        return {"scan": {v: k for k, v in GRU_SCAN.items()}[scan.value], "segments": seg.value, "steps": steps.value, "launches_per_eval": n.value,
                "workspace_bytes": ws.value}

    def plan_query(self, B, guided=False, split_phase=False):
        """The engine's plan for one denoiser evaluation of B motions: {class: dict(kernel, launches_per_eval, flops, l2_bytes)} for the
        classes that take part (rgn_plan_query: filled by the dispatching code itself)."""
        out = {}
        for i in range(32):
            name, kern, n, fl, l2 = C.c_char_p(), C.c_char_p(), C.c_double(), C.c_double(), C.c_double()
            code = self.lib.rgn_plan_query(self.h, int(B), int(bool(guided)), int(bool(split_phase)), i, C.byref(name), C.byref(kern),
                                           C.byref(n), C.byref(fl), C.byref(l2))
            if code != RGN_OK:
                break
            if kern.value:
                out[name.value.decode()] = {"kernel": kern.value.decode(), "launches_per_eval": n.value, "flops": fl.value, "l2_bytes": l2.value}
        if "gru_stack" in out:                                # the stack's own key also says which scan, how many segments and how much state
            info = self.gru_stack_info(B, guided)
            assert info["launches_per_eval"] == out["gru_stack"]["launches_per_eval"]
            out["gru_stack"].update(info)
        return out

    def randn(self, x, B, seed, sample_offset, stream):
        self._ck(self.lib.rgn_randn(self.h, _ptr(x), int(B), int(seed) & (2 ** 64 - 1), int(sample_offset), C.c_void_p(stream)))

    def randn_step(self, x, B, seed, sample_offset, loop_index, stream):
        """The fused loop's noise of loop index `loop_index` (-1: x_T) into x [B,njoints,nfeats,T]."""
        self._ck(self.lib.rgn_randn_step(self.h, _ptr(x), int(B), int(seed) & (2 ** 64 - 1), int(sample_offset), int(loop_index), C.c_void_p(stream)))

    def rot6d_to_matrix(self, d6, mat, n, stream):
        self._ck(self.lib.rgn_rot6d_to_matrix(self.h, _ptr(d6), _ptr(mat), int(n), C.c_void_p(stream)))

    def gaussian_filter1d(self, x, out, rows, T, sigma, stream):
        self._ck(self.lib.rgn_gaussian_filter1d(self.h, _ptr(x), _ptr(out), int(rows), int(T), float(sigma), C.c_void_p(stream)))

    def rot2xyz(self, x, mask, rest_joints, parents, pose_rep, num_person, flags, glob_rot, xyz, rotmat, stream):
        """rgn_rot2xyz: x fp32 [B, R, C * num_person, T] and mask (bool / uint8 [B, T] or None), contiguous on the engine's device -> xyz
        [B, J, 3 * num_person, T] (and rotmat [B, num_person, T, J, 3, 3] when given); rest_joints [J, 3] / parents [J] are host arrays."""
        rj = np.ascontiguousarray(rest_joints, dtype=np.float32)
        pa = np.ascontiguousarray(parents, dtype=np.int32)
        gr = None if glob_rot is None else np.ascontiguousarray(glob_rot, dtype=np.float32).reshape(3)
        assert rj.shape == (len(pa), 3) and x.is_contiguous() and xyz.is_contiguous() and (mask is None or (mask.is_contiguous() and mask.element_size() == 1))
        self._ck(self.lib.rgn_rot2xyz(self.h, _ptr(x), _ptr(mask), int(x.shape[0]), int(x.shape[-1]), len(pa), rj.ctypes.data_as(C.c_void_p),
                                      pa.ctypes.data_as(C.c_void_p), int(pose_rep), int(num_person), int(flags),
                                      None if gr is None else gr.ctypes.data_as(C.c_void_p), _ptr(xyz), _ptr(rotmat), C.c_void_p(stream)))

    def rot2xyz_shaped(self, x, mask, rest_joints, parents, shape_joints, betas, strides, pose_rep, num_person, flags, glob_rot, xyz, rotmat, stream):
        """rgn_rot2xyz_shaped: rot2xyz with shape_joints (fp32 [J, 3, nb]) and betas (fp32) on the engine's device; strides = (b, p, t) in elements
        of `betas`, 0 to broadcast."""
        rj = np.ascontiguousarray(rest_joints, dtype=np.float32)
        pa = np.ascontiguousarray(parents, dtype=np.int32)
        gr = None if glob_rot is None else np.ascontiguousarray(glob_rot, dtype=np.float32).reshape(3)
        assert rj.shape == (len(pa), 3) and x.is_contiguous() and xyz.is_contiguous() and (mask is None or (mask.is_contiguous() and mask.element_size() == 1))
        assert shape_joints.is_contiguous() and tuple(shape_joints.shape[:2]) == (len(pa), 3) and shape_joints.element_size() == betas.element_size() == 4
        sb, sp, st = (int(s) for s in strides)
        self._ck(self.lib.rgn_rot2xyz_shaped(self.h, _ptr(x), _ptr(mask), int(x.shape[0]), int(x.shape[-1]), len(pa), rj.ctypes.data_as(C.c_void_p),
                                             pa.ctypes.data_as(C.c_void_p), _ptr(shape_joints), int(shape_joints.shape[2]), _ptr(betas), sb, sp, st,
                                             int(pose_rep), int(num_person), int(flags), None if gr is None else gr.ctypes.data_as(C.c_void_p),
                                             _ptr(xyz), _ptr(rotmat), C.c_void_p(stream)))

    def loss_terms(self, target, output, cmotion, mask, rest_joints, parents, foot_joints, transl_row, vel_threshold, flags, terms, stream):
        """rgn_loss_terms: target / output / cmotion fp32 [B, J + 1, 6, T] and mask (bool / uint8 [B, T]), contiguous on the engine's device -> terms
        fp32 [B, 7] (columns: LOSS_TERMS); rest_joints [J, 3], parents [J] and foot_joints [4] are host arrays."""
        rj = np.ascontiguousarray(rest_joints, dtype=np.float32)
        pa = np.ascontiguousarray(parents, dtype=np.int32)
        fj = np.ascontiguousarray(foot_joints, dtype=np.int32).reshape(4)
        B, R, F, T = target.shape
        assert rj.shape == (len(pa), 3) and F == 6 and tuple(output.shape) == tuple(cmotion.shape) == (B, R, F, T)
        assert tuple(mask.shape) == (B, T) and mask.element_size() == 1 and tuple(terms.shape) == (B, len(LOSS_TERMS))
        assert all(a.is_contiguous() for a in (target, output, cmotion, mask, terms))
        self._ck(self.lib.rgn_loss_terms(self.h, _ptr(target), _ptr(output), _ptr(cmotion), _ptr(mask), int(B), int(T), int(R), len(pa),
                                         rj.ctypes.data_as(C.c_void_p), pa.ctypes.data_as(C.c_void_p), fj.ctypes.data_as(C.c_void_p), int(transl_row),
                                         float(vel_threshold), int(flags), _ptr(terms), C.c_void_p(stream)))

    def q_sample_rows(self, x_start, noise, coef, t, seed, sample_offset, x_t, noise_out, stream):
        """rgn_q_sample_rows: x_start fp32 [B, R, F, T], coef fp32 [N, 2], t int32 [N] -> x_t fp32 [N, R, F, T], row r of motion r % B; noise fp32
        [N, R, F, T], or None: drawn as rgn_randn_step(seed, sample_offset + b, t[r]) and, when noise_out is given, written there."""
        B, R, F, T = x_start.shape
        N = int(x_t.shape[0])
        assert tuple(x_t.shape) == (N, R, F, T) and tuple(coef.shape) == (N, 2) and tuple(t.shape) == (N,) and t.element_size() == 4
        assert all(a is None or (tuple(a.shape) == (N, R, F, T) and a.is_contiguous() and a.element_size() == 4) for a in (noise, noise_out))
        assert all(a.is_contiguous() and a.element_size() == 4 for a in (x_start, coef, t, x_t))
        self._ck(self.lib.rgn_q_sample_rows(self.h, _ptr(x_start), _ptr(noise), _ptr(coef), _ptr(t), int(B), N, int(R * F), int(T),
                                            int(seed) & (2 ** 64 - 1), int(sample_offset), _ptr(x_t), _ptr(noise_out), C.c_void_p(stream)))

    def vb_terms(self, x_start, x_t, output, noise, t, coef, flags, terms, stream):
        """rgn_vb_terms: x_start fp32 [B, R, F, T]; x_t, output and noise (or None) fp32 [N, R, F, T]; t int32 [N]; coef fp32 [N, 6] -> terms fp32
        [N, 3] (columns: VB_TERMS), row r of motion r % B."""
        B, R, F, T = x_start.shape
        N = int(x_t.shape[0])
        assert tuple(x_t.shape) == tuple(output.shape) == (N, R, F, T) and tuple(coef.shape) == (N, 6) and tuple(t.shape) == (N,) and t.element_size() == 4
        assert noise is None or (tuple(noise.shape) == (N, R, F, T) and noise.is_contiguous() and noise.element_size() == 4)
        assert tuple(terms.shape) == (N, len(VB_TERMS)) and all(a.is_contiguous() and a.element_size() == 4 for a in (x_start, x_t, output, coef, t, terms))
        self._ck(self.lib.rgn_vb_terms(self.h, _ptr(x_start), _ptr(x_t), _ptr(output), _ptr(noise), _ptr(t), _ptr(coef), int(B), N, int(R * F), int(T),
                                       int(flags), _ptr(terms), C.c_void_p(stream)))

    def hml_to_joints(self, x, mean, std, joints, xyz, stream):
        """rgn_hml_to_joints: x fp32 [B, 12 J - 1, 1, T] (a HumanML3D / KIT sample in the model's layout), mean / std fp32 [12 J - 1] or both None,
        contiguous on the engine's device -> xyz fp32 [B, J, 3, T], which must not share memory with x."""
        B, D, F, T = x.shape
        assert F == 1 and tuple(xyz.shape) == (B, int(joints), 3, T) and (mean is None) == (std is None)
        assert all(a is None or (a.is_contiguous() and a.element_size() == 4) for a in (x, mean, std, xyz))
        assert mean is None or tuple(mean.shape) == tuple(std.shape) == (D,)
        self._ck(self.lib.rgn_hml_to_joints(self.h, _ptr(x), _ptr(mean), _ptr(std), int(B), int(T), int(D), int(joints), _ptr(xyz), C.c_void_p(stream)))

    def profile_enable(self, on):
        self._ck(self.lib.rgn_profile_enable(self.h, int(bool(on))))

    def profile_bracket_overhead_ms(self):
        ms = C.c_double()
        self._ck(self.lib.rgn_profile_bracket_overhead(self.h, C.byref(ms)))
        return ms.value

    def profile_query(self):
        out = {}
        for i in range(16):
            name, ms, n = C.c_char_p(), C.c_double(), C.c_int64()
            code = self.lib.rgn_profile_query(self.h, i, C.byref(name), C.byref(ms), C.byref(n))
            if code != RGN_OK:
                break
            out[name.value.decode()] = (ms.value, n.value)
        return out


def _block_arrays(blocks):
    blocks = [(int(co), int(st)) for co, st in blocks]
    n = max(len(blocks), 1)
    return (C.c_int32 * n)(*[b[0] for b in blocks]), (C.c_int32 * n)(*[b[1] for b in blocks])


def check_stgcn_blocks(blocks):
    """rgn_stgcn_check_blocks: the block-plan rules of rgn_stgcn_set_blocks without a handle or a device. Raises RgnError (RGN_ERR_INVALID_ARG, the
    offending entry named) for a plan the engine does not take."""
    co, st = _block_arrays(blocks)
    err = C.create_string_buffer(512)
    code = load().rgn_stgcn_check_blocks(len(blocks), co, st, err, 512)
    if code != RGN_OK:
        raise RgnError(code, err.value.decode())


class StgcnEngine:
    """Owns one rgn_stgcn_handle (the ST-GCN evaluator, include/regennet_hip.h)."""

    def __init__(self, in_channels, num_class, num_person, num_nodes, num_frames, max_batch, device_index, options=None, blocks=None):
        """blocks: [(out_channels, stride), ...] of the st_gcn blocks (rgn_stgcn_set_blocks); None: the reference's ten."""
        self.lib = load()
        self.shape = (int(num_nodes), int(in_channels), int(num_frames))
        self.num_class, self.max_batch = int(num_class), int(max_batch)
        cfg = RgnStgcnConfig(in_channels=in_channels, num_class=num_class, num_person=num_person, num_nodes=num_nodes,
                             num_frames=num_frames, max_batch=max_batch, device=int(device_index))
        h = C.c_void_p()
        code = self.lib.rgn_stgcn_create(C.byref(cfg), C.byref(h))
        if code != RGN_OK:
            raise RgnError(code, (self.lib.rgn_stgcn_last_error(None) or b"").decode())
        self.h = h
        for k, v in (options or {}).items():         # kernel-selection switches of this handle (rgn_stgcn_set_option)
            self.set_option(k, v)
        if blocks is not None:
            try:
                self.set_blocks(blocks)
            except Exception:
                self.close()
                raise

    def _ck(self, code):
        if code != RGN_OK:
            raise RgnError(code, (self.lib.rgn_stgcn_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.rgn_stgcn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_weight(self, key, array):
        a = np.ascontiguousarray(array, dtype=np.float32)
        shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
        self._ck(self.lib.rgn_stgcn_load_weight(self.h, key.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))

    def set_blocks(self, blocks):
        co, st = _block_arrays(blocks)
        self._ck(self.lib.rgn_stgcn_set_blocks(self.h, len(blocks), co, st))

    def finalize(self):
        self._ck(self.lib.rgn_stgcn_finalize(self.h))

    def set_option(self, key, value):
        self._ck(self.lib.rgn_stgcn_set_option(self.h, key.encode(), int(value)))

    def forward(self, N, output, features, yhat, stream):
        self._ck(self.lib.rgn_stgcn_forward(self.h, int(N), _ptr(output), _ptr(features), _ptr(yhat), C.c_void_p(stream)))


class GruEngine:
    """Owns one rgn_gru_handle (the GRU action classifier of the action2motion evaluation, include/regennet_hip.h)."""

    def __init__(self, input_size, hidden_size, num_layers, lin1_size, output_size, device_index):
        self.lib = load()
        self.input_size, self.hidden_size, self.num_layers = int(input_size), int(hidden_size), int(num_layers)
        self.lin1_size, self.output_size = int(lin1_size), int(output_size)
        cfg = RgnGruConfig(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers, lin1_size=lin1_size,
                           output_size=output_size, device=int(device_index))
        h = C.c_void_p()
        code = self.lib.rgn_gru_create(C.byref(cfg), C.byref(h))
        if code != RGN_OK:
            raise RgnError(code, (self.lib.rgn_gru_last_error(None) or b"").decode())
        self.h = h

    def _ck(self, code):
        if code != RGN_OK:
            raise RgnError(code, (self.lib.rgn_gru_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.rgn_gru_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_weight(self, key, array):
        a = np.ascontiguousarray(array, dtype=np.float32)
        shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
        self._ck(self.lib.rgn_gru_load_weight(self.h, key.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))

    def finalize(self):
        self._ck(self.lib.rgn_gru_finalize(self.h))

    def forward(self, N, T, x, lengths, h0, features, logits, stream):
        self._ck(self.lib.rgn_gru_forward(self.h, int(N), int(T), _ptr(x), _ptr(lengths), _ptr(h0), _ptr(features), _ptr(logits), C.c_void_p(stream)))

    def lengths_clamped(self):
        """True when a forward since the last query met a length outside [1, T] (it was clamped). Synchronises the device."""
        v = C.c_int32(0)
        self._ck(self.lib.rgn_gru_length_status(self.h, C.byref(v)))
        return bool(v.value)


T2M_FIELDS = ("dim_pose", "movement_hidden", "movement_latent", "motion_hidden", "dim_word", "dim_pos_ohot", "text_hidden", "coemb", "unit_length")


class T2mEngine:
    """Owns one rgn_t2m_handle (the text-to-motion evaluator: movement encoder and the two bi-GRU co-embedding encoders, include/regennet_hip.h) and
    the workspace its calls share, grown on demand."""

    def __init__(self, geometry, device_index):
        import torch
        self.lib = load()
        self.geometry = {k: int(geometry[k]) for k in T2M_FIELDS}
        self.device = torch.device("cuda", int(device_index))
        cfg = RgnT2mConfig(device=int(device_index), **self.geometry)
        h = C.c_void_p()
        code = self.lib.rgn_t2m_create(C.byref(cfg), C.byref(h))
        if code != RGN_OK:
            raise RgnError(code, (self.lib.rgn_t2m_last_error(None) or b"").decode())
        self.h = h
        self._work = None

    def _ck(self, code):
        if code != RGN_OK:
            raise RgnError(code, (self.lib.rgn_t2m_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.rgn_t2m_destroy(self.h)
            self.h = None
            self._work = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_weight(self, key, array):
        a = np.ascontiguousarray(array, dtype=np.float32)
        shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
        self._ck(self.lib.rgn_t2m_load_weight(self.h, key.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))

    def finalize(self):
        self._ck(self.lib.rgn_t2m_finalize(self.h))

    def workspace_bytes(self, N, T, Lw):
        v = C.c_size_t(0)
        self._ck(self.lib.rgn_t2m_workspace(self.h, int(N), int(T), int(Lw), C.byref(v)))
        return int(v.value)

    def _workspace(self, N, T, Lw):
        import torch
        need = self.workspace_bytes(N, T, Lw)
        if self._work is None or self._work.numel() < need:
            if self._work is not None:
                torch.cuda.synchronize(self.device)       # a kernel of an earlier call may still be using the old buffer
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._work

    def movements(self, N, T, in_stride, x, m_lens, out, stream):
        w = self._workspace(N, T, 1)
        self._ck(self.lib.rgn_t2m_movements(self.h, int(N), int(T), int(in_stride), _ptr(x), _ptr(m_lens), _ptr(out), _ptr(w), w.numel(), C.c_void_p(stream)))

    def encode_movements(self, N, T2, mov, lens, out, stream):
        w = self._workspace(N, 4 * T2, 1)
        self._ck(self.lib.rgn_t2m_encode_movements(self.h, int(N), int(T2), _ptr(mov), _ptr(lens), _ptr(out), _ptr(w), w.numel(), C.c_void_p(stream)))

    def motion_embeddings(self, N, T, motions, m_lens, out, stream):
        w = self._workspace(N, T, 1)
        self._ck(self.lib.rgn_t2m_motion_embeddings(self.h, int(N), int(T), _ptr(motions), _ptr(m_lens), _ptr(out), _ptr(w), w.numel(), C.c_void_p(stream)))

    def text_embeddings(self, N, Lw, word_embs, pos_ohot, cap_lens, out, stream):
        w = self._workspace(N, 4, Lw)
        self._ck(self.lib.rgn_t2m_text_embeddings(self.h, int(N), int(Lw), _ptr(word_embs), _ptr(pos_ohot), _ptr(cap_lens), _ptr(out), _ptr(w), w.numel(),
                                                  C.c_void_p(stream)))

    def lengths_clamped(self):
        """True when a call since the last query met a length outside its range (it was clamped). Synchronises the device."""
        v = C.c_int32(0)
        self._ck(self.lib.rgn_t2m_length_status(self.h, C.byref(v)))
        return bool(v.value)


def t2m_match(text, motion, group=32):
    """(diag fp32 [N], rank int32 [N]) of rgn_t2m_match for device tensors text, motion [N, D]: the distance of every true pair and the number of
    motions of its group of `group` strictly nearer to the text. Top-k hit <=> rank < k."""
    import torch
    lib = load()
    N, D = text.shape
    if motion.shape != text.shape:
        raise ValueError(f"text {tuple(text.shape)} and motion {tuple(motion.shape)} differ")
    text, motion = text.float().contiguous(), motion.float().contiguous()
    diag = torch.empty(N, dtype=torch.float32, device=text.device)
    rank = torch.empty(N, dtype=torch.int32, device=text.device)
    code = lib.rgn_t2m_match(text.device.index or 0, _ptr(text), _ptr(motion), int(N), int(D), int(group), _ptr(diag), _ptr(rank),
                             C.c_void_p(torch.cuda.current_stream(text.device).cuda_stream))
    if code != RGN_OK:
        raise RgnError(code, (lib.rgn_t2m_last_error(None) or b"").decode())
    return diag, rank


def _host(a, dtype):
    """(contiguous array or None, its pointer or None): the array must outlive the call."""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(C.c_void_p)


class BodyEngine:
    """Owns one rgn_body_handle: the mesh data of a body file on one device (include/regennet_hip.h). `mesh`: the dict
    model.rotation2xyz.check_body returns under 'mesh'; J: the skeleton's joint count."""

    def __init__(self, mesh, J, device_index):
        self.lib = load()
        vt, pt = _host(mesh["v_template"], np.float32)
        pd, pp = _host(mesh.get("posedirs"), np.float32)
        w, pw = _host(mesh["lbs_weights"], np.float32)
        sd, ps = _host(mesh.get("shapedirs"), np.float32)
        ij = mesh.get("identity_joints", None)
        idj, pi = _host(() if ij is None else ij, np.int32)
        self.V, self.J, self.nb = int(vt.shape[0]), int(J), 0 if sd is None else int(sd.shape[2])
        h = C.c_void_p()
        code = self.lib.rgn_body_create(int(device_index), self.V, self.J, self.nb, pt, pp, pw, ps, pi if len(idj) else None, len(idj), C.byref(h))
        if code != RGN_OK:
            raise RgnError(code, (self.lib.rgn_body_last_error(None) or b"").decode())
        self.h = h

    def _ck(self, code):
        if code != RGN_OK:
            raise RgnError(code, (self.lib.rgn_body_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.rgn_body_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self, B, T, num_person):
        n = C.c_uint64()
        self._ck(self.lib.rgn_rot2verts_workspace(self.h, int(B), int(T), int(num_person), C.byref(n)))
        return n.value

    def rot2verts(self, x, mask, rest_joints, parents, pose_rep, num_person, flags, glob_rot, betas, verts, rotmat, work, stream):
        """rgn_rot2verts: x fp32 [B, R, C * num_person, T] and mask (bool / uint8 [B, T] or None), contiguous on the body's device -> verts
        [B, V, 3 * num_person, T] (and rotmat [B, num_person, T, J, 3, 3] when given); rest_joints [J, 3], parents [J], betas [nb] | None are host
        arrays; work: a uint8 tensor of at least workspace_bytes(B, T, num_person)."""
        rj, prj = _host(rest_joints, np.float32)
        pa, ppa = _host(parents, np.int32)
        gr, pgr = _host(None if glob_rot is None else np.asarray(glob_rot).reshape(3), np.float32)
        be, pbe = _host(betas, np.float32)
        assert rj.shape == (self.J, 3) and pa.shape == (self.J,) and (be is None or be.shape == (self.nb,))
        assert x.is_contiguous() and verts.is_contiguous() and (mask is None or (mask.is_contiguous() and mask.element_size() == 1))
        self._ck(self.lib.rgn_rot2verts(self.h, _ptr(x), _ptr(mask), int(x.shape[0]), int(x.shape[-1]), prj, ppa, int(pose_rep), int(num_person),
                                        int(flags), pgr, pbe, _ptr(verts), _ptr(rotmat), _ptr(work), int(work.numel() * work.element_size()),
                                        C.c_void_p(stream)))

    def workspace_bytes_shaped(self, B, T, num_person):
        n = C.c_uint64()
        self._ck(self.lib.rgn_rot2verts_shaped_workspace(self.h, int(B), int(T), int(num_person), C.byref(n)))
        return n.value

    def rot2verts_shaped(self, x, mask, rest_joints, parents, shape_joints, betas, strides, pose_rep, num_person, flags, glob_rot, verts, rotmat, work,
                         stream):
        """rgn_rot2verts_shaped: rot2verts with shape_joints (fp32 [J, 3, nb], nb <= self.nb) and betas (fp32) on the body's device; strides =
        (b, p, t) in elements of `betas`, 0 to broadcast; rest_joints: the file's, without betas; work: a uint8 tensor of at least
        workspace_bytes_shaped(B, T, num_person)."""
        rj, prj = _host(rest_joints, np.float32)
        pa, ppa = _host(parents, np.int32)
        gr, pgr = _host(None if glob_rot is None else np.asarray(glob_rot).reshape(3), np.float32)
        assert rj.shape == (self.J, 3) and pa.shape == (self.J,)
        assert x.is_contiguous() and verts.is_contiguous() and (mask is None or (mask.is_contiguous() and mask.element_size() == 1))
        assert shape_joints.is_contiguous() and tuple(shape_joints.shape[:2]) == (self.J, 3) and shape_joints.element_size() == betas.element_size() == 4
        sb, sp, st = (int(s) for s in strides)
        self._ck(self.lib.rgn_rot2verts_shaped(self.h, _ptr(x), _ptr(mask), int(x.shape[0]), int(x.shape[-1]), prj, ppa, _ptr(shape_joints),
                                               int(shape_joints.shape[2]), _ptr(betas), sb, sp, st, int(pose_rep), int(num_person), int(flags), pgr,
                                               _ptr(verts), _ptr(rotmat), _ptr(work), int(work.numel() * work.element_size()), C.c_void_p(stream)))

    def set_joint_regressors(self, vertex_joints, regressor):
        """rgn_body_set_joint_regressors: vertex_joints int [Np] | None, regressor fp32 [Jr, V] | None (host). The body is cut to the vertices
        they touch, once; a second call replaces the data."""
        vj, pvj = _host(() if vertex_joints is None else vertex_joints, np.int32)
        reg, preg = _host(np.zeros((0, self.V), np.float32) if regressor is None else regressor, np.float32)
        assert vj.ndim == 1 and reg.ndim == 2 and reg.shape[1] == self.V, (vj.shape, reg.shape, self.V)
        self._ck(self.lib.rgn_body_set_joint_regressors(self.h, len(vj), pvj if len(vj) else None, len(reg), preg if len(reg) else None))
        self.Np, self.Jr = len(vj), len(reg)

    def joints_workspace_bytes(self, B, T, num_person):
        n = C.c_uint64()
        self._ck(self.lib.rgn_rot2joints_workspace(self.h, int(B), int(T), int(num_person), C.byref(n)))
        return n.value

    def joints_workspace_bytes_shaped(self, B, T, num_person):
        n = C.c_uint64()
        self._ck(self.lib.rgn_rot2joints_shaped_workspace(self.h, int(B), int(T), int(num_person), C.byref(n)))
        return n.value

    def rot2joints(self, x, mask, rest_joints, parents, pose_rep, num_person, flags, glob_rot, betas, jmap, root, joints, rotmat, work, stream):
        """rgn_rot2joints: rot2verts's arguments, with in place of verts the joint type - jmap int [n] into [J chain joints | Np picked | Jr
        regressed] (host), root (an output row) - and joints fp32 [B, n, 3 * num_person, T]; work: at least joints_workspace_bytes(...)."""
        rj, prj = _host(rest_joints, np.float32)
        pa, ppa = _host(parents, np.int32)
        gr, pgr = _host(None if glob_rot is None else np.asarray(glob_rot).reshape(3), np.float32)
        be, pbe = _host(betas, np.float32)
        jm, pjm = _host(np.asarray(jmap).reshape(-1), np.int32)
        assert rj.shape == (self.J, 3) and pa.shape == (self.J,) and (be is None or be.shape == (self.nb,))
        assert x.is_contiguous() and joints.is_contiguous() and (mask is None or (mask.is_contiguous() and mask.element_size() == 1))
        assert tuple(joints.shape[1:3]) == (len(jm), 3 * int(num_person)), (tuple(joints.shape), len(jm), num_person)
        self._ck(self.lib.rgn_rot2joints(self.h, _ptr(x), _ptr(mask), int(x.shape[0]), int(x.shape[-1]), prj, ppa, int(pose_rep), int(num_person),
                                         int(flags), pgr, pbe, len(jm), pjm, int(root), _ptr(joints), _ptr(rotmat), _ptr(work),
                                         int(work.numel() * work.element_size()), C.c_void_p(stream)))

    def rot2joints_shaped(self, x, mask, rest_joints, parents, shape_joints, betas, strides, pose_rep, num_person, flags, glob_rot, jmap, root, joints,
                          rotmat, work, stream):
        """rgn_rot2joints_shaped: rot2joints with the shape arguments of rot2verts_shaped; work: at least joints_workspace_bytes_shaped(...)."""
        rj, prj = _host(rest_joints, np.float32)
        pa, ppa = _host(parents, np.int32)
        gr, pgr = _host(None if glob_rot is None else np.asarray(glob_rot).reshape(3), np.float32)
        jm, pjm = _host(np.asarray(jmap).reshape(-1), np.int32)
        assert rj.shape == (self.J, 3) and pa.shape == (self.J,)
        assert x.is_contiguous() and joints.is_contiguous() and (mask is None or (mask.is_contiguous() and mask.element_size() == 1))
        assert tuple(joints.shape[1:3]) == (len(jm), 3 * int(num_person)), (tuple(joints.shape), len(jm), num_person)
        assert shape_joints.is_contiguous() and tuple(shape_joints.shape[:2]) == (self.J, 3) and shape_joints.element_size() == betas.element_size() == 4
        sb, sp, st = (int(s) for s in strides)
        self._ck(self.lib.rgn_rot2joints_shaped(self.h, _ptr(x), _ptr(mask), int(x.shape[0]), int(x.shape[-1]), prj, ppa, _ptr(shape_joints),
                                                int(shape_joints.shape[2]), _ptr(betas), sb, sp, st, int(pose_rep), int(num_person), int(flags), pgr,
                                                len(jm), pjm, int(root), _ptr(joints), _ptr(rotmat), _ptr(work),
                                                int(work.numel() * work.element_size()), C.c_void_p(stream)))


class RenderEngine:
    """Owns one rgn_render_handle: the faces of one mesh topology (and the vertex -> face adjacency built from them) on one device."""

    def __init__(self, faces, V, device_index):
        self.lib = load()
        f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        self.V, self.F = int(V), int(f.shape[0])
        h = C.c_void_p()
        code = self.lib.rgn_render_create(int(device_index), self.V, self.F, f.ctypes.data_as(C.c_void_p), C.byref(h))
        if code != RGN_OK:
            raise RgnError(code, (self.lib.rgn_render_last_error(None) or b"").decode())
        self.h = h

    def _ck(self, code):
        if code != RGN_OK:
            raise RgnError(code, (self.lib.rgn_render_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.rgn_render_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self, B, T, num_person, width, height):
        n = C.c_uint64()
        self._ck(self.lib.rgn_render_workspace(self.h, int(B), int(T), int(num_person), int(width), int(height), C.byref(n)))
        return n.value

    @staticmethod
    def params(width, height, cam, center, colors, background):
        """rgn_render_params from plain sequences; `colors`: one (r, g, b) per person, the last repeated up to the struct's RENDER_MAX_PERSONS."""
        p = RgnRenderParams(width=int(width), height=int(height), center=int(bool(center)))
        p.cam[:] = [float(c) for c in cam]
        colors = [tuple(float(x) for x in c) for c in colors]
        for i in range(RENDER_MAX_PERSONS):
            p.colors[i][:] = colors[min(i, len(colors) - 1)]
        p.background[:] = [float(c) for c in background]
        return p

    def render(self, verts, mask, num_person, params, rgb, depth, face, work, stream):
        """rgn_render: verts fp32 [B, V, 3 * num_person, T] and mask (bool / uint8 [B, T] or None), contiguous on the renderer's device -> rgb uint8
        [B, T, H, W, 3] (and depth fp32 / face int32 [B, T, H, W] when given); work: a uint8 tensor of at least workspace_bytes(...)."""
        assert verts.is_contiguous() and rgb.is_contiguous() and (mask is None or (mask.is_contiguous() and mask.element_size() == 1))
        assert tuple(verts.shape[1:3]) == (self.V, 3 * int(num_person)), (tuple(verts.shape), self.V, num_person)
        self._ck(self.lib.rgn_render(self.h, _ptr(verts), _ptr(mask), int(verts.shape[0]), int(verts.shape[-1]), int(num_person), C.byref(params),
                                     _ptr(rgb), _ptr(depth), _ptr(face), _ptr(work), int(work.numel() * work.element_size()), C.c_void_p(stream)))
