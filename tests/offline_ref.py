"""fp32 CPU restatement of the reference's arch='offline' denoiser (model/cmdm.py:228-238), built from torch.nn.TransformerEncoderLayer
and the state dict, for shapes the recorded goldens do not cover. A test checker only (tests/test_offline_cpu.py pins it to the
goldens recorded from the reference itself); sampling loops reuse oracle.regennet_oracle.sample_loop with cmdm_forward patched to
this forward."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def _t(sd, k):
    return torch.as_tensor(sd[k], dtype=torch.float32)


def _encoder(sd, cfg):
    """nn.TransformerEncoder of cfg['layers'] post-norm nn.TransformerEncoderLayers (gelu, eps 1e-5, no final norm) holding the
    checkpoint's seqTransEncoder.* tensors - the module the reference builds (model/cmdm.py:63-71)."""
    layer = nn.TransformerEncoderLayer(d_model=cfg["latent_dim"], nhead=cfg["num_heads"], dim_feedforward=cfg["ff_size"], dropout=0.1,
                                       activation="gelu")
    enc = nn.TransformerEncoder(layer, num_layers=cfg["layers"], enable_nested_tensor=False)
    p = "seqTransEncoder."
    enc.load_state_dict({k[len(p):]: _t(sd, k) for k in sd if k.startswith(p)}, strict=True)
    return enc.eval()


def cmdm_forward(sd, cfg, x, timesteps, y):
    """x [B,J,F,T] fp32, timesteps [B] int64 (original indices), y dict -> x0_hat [B,J,F,T]."""
    B, J, Fe, T = x.shape
    pe = _t(sd, "sequence_pos_encoder.pe")
    with torch.no_grad():
        emb = F.linear(F.silu(F.linear(pe[timesteps], _t(sd, "embed_timestep.time_embed.0.weight"), _t(sd, "embed_timestep.time_embed.0.bias"))),
                       _t(sd, "embed_timestep.time_embed.2.weight"), _t(sd, "embed_timestep.time_embed.2.bias")).permute(1, 0, 2)
        force_mask = y.get("uncond", False)
        if "text" in cfg["cond_mode"]:
            enc = y["text_features"]
            emb = emb + F.linear(torch.zeros_like(enc) if force_mask else enc, _t(sd, "embed_text.weight"), _t(sd, "embed_text.bias"))
        if "action" in cfg["cond_mode"]:
            a = _t(sd, "embed_action.action_embedding")[y["action"][:, 0].long()]
            emb = emb + (torch.zeros_like(a) if force_mask else a)
        xs = F.linear(x.permute(3, 0, 1, 2).reshape(T, B, J * Fe), _t(sd, "input_process.poseEmbedding.weight"), _t(sd, "input_process.poseEmbedding.bias"))
        cs = F.linear(y["cmotion"].permute(3, 0, 1, 2).reshape(T, B, J * Fe), _t(sd, "cmo_process.poseEmbedding.weight"),
                      _t(sd, "cmo_process.poseEmbedding.bias"))
        if cfg["cm_mode"] == "add":
            xseq = xs + cs
        else:
            xseq = F.linear(torch.cat((xs, cs), dim=-1), _t(sd, "fuse_process.weight"), _t(sd, "fuse_process.bias"))
        xseq = torch.cat((emb, xseq), dim=0)                 # the embedding is token 0, always
        xseq = xseq + pe[: xseq.shape[0]]                    # positions always encoded
        xseq = _encoder(sd, cfg)(xseq)                       # full self-attention, post-norm, no final norm
        out = F.linear(xseq[1:], _t(sd, "output_process.poseFinal.weight"), _t(sd, "output_process.poseFinal.bias"))
    return out.reshape(T, B, J, Fe).permute(1, 2, 3, 0)


def cfg_forward(sd, cfg, x, timesteps, y):
    """ClassifierFreeSampleModel.forward around the offline forward."""
    out = cmdm_forward(sd, cfg, x, timesteps, y)
    out_u = cmdm_forward(sd, cfg, x, timesteps, dict(y, uncond=True))
    return out_u + y["scale"].view(-1, 1, 1, 1) * (out - out_u)
