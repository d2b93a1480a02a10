"""fp32 CPU restatement of the reference's arch='mlp' denoiser (model/cmdm.py:239-242 around the DiffMLP of model/mlp.py:9-86), written from
the formulas and the state dict. A test checker only (tests/test_mlp_arch_cpu.py pins it to the goldens recorded from the reference
itself); sampling loops and the scoring functions take it as the model.

    h = conct(cat(c_in, x_in))                           Linear(2d, d), block 0 only; the ACTOR half first
    for every block l:
        h = h + emb_fc_l(SiLU(emb))                      a [B, d] vector, broadcast over frames
        h = h + SiLU(W0_l . LN0_l(h) + b0_l[:, None])    W0_l [T, T] contracts over FRAMES, b0_l per output frame
        h = h + SiLU(LN1_l(h) . W1_l^T + b1_l)           [d, d]
    out = output_process(h)

No positional encoding, cm_mode is not read, lengths / mask are not read."""
import torch
import torch.nn.functional as F


def _t(sd, k):
    return torch.as_tensor(sd[k], dtype=torch.float32)


def embedding(sd, cfg, timesteps, y):
    """emb [B, d]: embed_timestep(t) + the condition embedding (zeroed / embed_text(0) under y['uncond'])."""
    pe = _t(sd, "sequence_pos_encoder.pe")[:, 0]
    emb = F.linear(F.silu(F.linear(pe[timesteps], _t(sd, "embed_timestep.time_embed.0.weight"), _t(sd, "embed_timestep.time_embed.0.bias"))),
                   _t(sd, "embed_timestep.time_embed.2.weight"), _t(sd, "embed_timestep.time_embed.2.bias"))
    force_mask = y.get("uncond", False)
    if "text" in cfg["cond_mode"]:
        enc = y["text_features"]
        emb = emb + F.linear(torch.zeros_like(enc) if force_mask else enc, _t(sd, "embed_text.weight"), _t(sd, "embed_text.bias"))
    if "action" in cfg["cond_mode"]:
        a = _t(sd, "embed_action.action_embedding")[y["action"][:, 0].long()]
        emb = emb + (torch.zeros_like(a) if force_mask else a)
    return emb


def mixer_stack(sd, cfg, h, emb):
    """h [B, T, d] (block 0's conct already applied), emb [B, d] -> [B, T, d]."""
    d = cfg["latent_dim"]
    for l in range(cfg["layers"]):
        p = f"mlp.motion_mlp.mlps.{l}."
        h = h + F.linear(F.silu(emb), _t(sd, p + "emb_fc.weight"), _t(sd, p + "emb_fc.bias"))[:, None, :]
        u = F.layer_norm(h, (d,), _t(sd, p + "norm0.weight"), _t(sd, p + "norm0.bias"), 1e-5)
        w0 = _t(sd, p + "fc0.weight")[:, :, 0]
        h = h + F.silu(torch.einsum("st,btd->bsd", w0, u) + _t(sd, p + "fc0.bias")[None, :, None])
        w = F.layer_norm(h, (d,), _t(sd, p + "norm1.weight"), _t(sd, p + "norm1.bias"), 1e-5)
        h = h + F.silu(F.linear(w, _t(sd, p + "fc1.weight"), _t(sd, p + "fc1.bias")))
    return h


def cmdm_forward(sd, cfg, x, timesteps, y):
    """x [B,J,F,T] fp32, timesteps [B] int64 (original indices), y dict -> x0_hat [B,J,F,T]."""
    B, J, Fe, T = x.shape
    if T != cfg["num_frames"]:
        raise ValueError(f"fc0 mixes exactly num_frames = {cfg['num_frames']} frames, not {T}")
    with torch.no_grad():
        emb = embedding(sd, cfg, timesteps, y)
        xs = F.linear(x.permute(0, 3, 1, 2).reshape(B, T, J * Fe), _t(sd, "input_process.poseEmbedding.weight"), _t(sd, "input_process.poseEmbedding.bias"))
        cs = F.linear(y["cmotion"].to(x.dtype).permute(0, 3, 1, 2).reshape(B, T, J * Fe), _t(sd, "cmo_process.poseEmbedding.weight"),
                      _t(sd, "cmo_process.poseEmbedding.bias"))
        p0 = "mlp.motion_mlp.mlps.0."
        h = F.linear(torch.cat((cs, xs), dim=-1), _t(sd, p0 + "conct.weight"), _t(sd, p0 + "conct.bias"))
        h = mixer_stack(sd, cfg, h, emb)
        out = F.linear(h, _t(sd, "output_process.poseFinal.weight"), _t(sd, "output_process.poseFinal.bias"))
    return out.reshape(B, T, J, Fe).permute(0, 2, 3, 1)


def cfg_forward(sd, cfg, x, timesteps, y):
    """ClassifierFreeSampleModel.forward around the mlp forward."""
    out = cmdm_forward(sd, cfg, x, timesteps, y)
    out_u = cmdm_forward(sd, cfg, x, timesteps, dict(y, uncond=True))
    return out_u + y["scale"].view(-1, 1, 1, 1) * (out - out_u)
