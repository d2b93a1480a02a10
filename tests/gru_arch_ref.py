"""CPU restatement of the reference's arch='gru' denoiser (model/cmdm.py:191-199, 243-249), written from the equations and the state dict, in fp32
or fp64. A test checker only (tests/test_gru_arch_cpu.py pins it to the goldens recorded from the reference itself); sampling loops take it as the
model.

    emb  [B, d]    = embed_timestep(t) [+ masked action / text embedding]
    x_in [T, B, d] = W_x [x_tb ; emb_b] + b_x            input_process.poseEmbedding [d, F + d]
    c_in [T, B, d] = W_c [c_tb ; emb_b] + b_c            cmo_process.poseEmbedding   [d, F + d]
    xseq           = c_in + x_in + pe[t]                 cm_mode 'add' only, no fuse_process
    out            = GRU(d, d, L layers, zero initial state)(xseq)
    x0             = output_process(out)

scan='batch' is the reference's own recurrence: it hands xseq [T, B, d] to a batch_first nn.GRU, which takes the T frames as its batch and scans
the B samples. scan='frames' scans the frames of every sample. One GRU cell, gate order r, z, n:

    r = s(W_ir x + b_ir + W_hr h + b_hr),  z likewise,  n = tanh(W_in x + b_in + r (W_hn h + b_hn)),  h' = (1 - z) n + z h

`mutant` names one deliberate mistake (tests/test_gru_arch_cpu.py checks that each breaks the GPU bound on some fixture)."""
import torch
import torch.nn.functional as F

MUTANTS = ("other_axis", "no_restart", "stale_state", "r_without_bhn", "no_cmo_emb", "no_pe")


def _t(sd, k, dtype):
    return torch.as_tensor(sd[k]).to(dtype)


def embedding(sd, cfg, timesteps, y, dtype=torch.float32):
    """emb [B, d]: embed_timestep(t) + the condition embedding (zeroed / embed_text(0) under y['uncond'])."""
    pe = _t(sd, "sequence_pos_encoder.pe", dtype)[:, 0]
    emb = F.linear(F.silu(F.linear(pe[timesteps], _t(sd, "embed_timestep.time_embed.0.weight", dtype), _t(sd, "embed_timestep.time_embed.0.bias", dtype))),
                   _t(sd, "embed_timestep.time_embed.2.weight", dtype), _t(sd, "embed_timestep.time_embed.2.bias", dtype))
    force_mask = y.get("uncond", False)
    if "text" in cfg["cond_mode"]:
        enc = torch.as_tensor(y["text_features"]).to(dtype)
        emb = emb + F.linear(torch.zeros_like(enc) if force_mask else enc, _t(sd, "embed_text.weight", dtype), _t(sd, "embed_text.bias", dtype))
    if "action" in cfg["cond_mode"]:
        a = _t(sd, "embed_action.action_embedding", dtype)[torch.as_tensor(y["action"])[:, 0].long()]
        emb = emb + (torch.zeros_like(a) if force_mask else a)
    return emb


def gru_stack(sd, cfg, xs, dtype=torch.float32, mutant=None):
    """xs [S, N, d]: S steps of N independent sequences -> the top layer's state at every step [S, N, d]. Zero initial state."""
    d = cfg["latent_dim"]
    S, N = xs.shape[:2]
    for l in range(cfg["layers"]):
        w_ih, w_hh = _t(sd, f"gru.weight_ih_l{l}", dtype), _t(sd, f"gru.weight_hh_l{l}", dtype)
        b_ih, b_hh = _t(sd, f"gru.bias_ih_l{l}", dtype), _t(sd, f"gru.bias_hh_l{l}", dtype)
        h = torch.zeros(N, d, dtype=dtype)
        older = torch.zeros(N, d, dtype=dtype)
        outs = []
        for s in range(S):
            src = older if mutant == "stale_state" else h               # (the mutant reads the state of two steps back)
            gi = F.linear(xs[s], w_ih, b_ih)
            if mutant == "r_without_bhn":
                gh = F.linear(src, w_hh)
                gh[:, : 2 * d] += b_hh[: 2 * d]
            else:
                gh = F.linear(src, w_hh, b_hh)
            r = torch.sigmoid(gi[:, :d] + gh[:, :d])
            z = torch.sigmoid(gi[:, d:2 * d] + gh[:, d:2 * d])
            hn = r * gh[:, 2 * d:]
            if mutant == "r_without_bhn":
                hn = hn + b_hh[2 * d:]
            n = torch.tanh(gi[:, 2 * d:] + hn)
            older = h
            h = (1.0 - z) * n + z * src
            outs.append(h)
        xs = torch.stack(outs)
    return xs


def xseq_of(sd, cfg, x, timesteps, y, dtype=torch.float32, mutant=None):
    """The GRU's input [B, T, d] (sample-major)."""
    B, J, Fe, T = x.shape
    Fin = J * Fe
    emb = embedding(sd, cfg, timesteps, y, dtype)
    xr = x.to(dtype).permute(0, 3, 1, 2).reshape(B, T, Fin)
    cr = torch.as_tensor(y["cmotion"]).to(dtype).permute(0, 3, 1, 2).reshape(B, T, Fin)
    e = emb[:, None, :].expand(B, T, emb.shape[1])
    x_in = F.linear(torch.cat((xr, e), dim=-1), _t(sd, "input_process.poseEmbedding.weight", dtype), _t(sd, "input_process.poseEmbedding.bias", dtype))
    ce = torch.zeros_like(e) if mutant == "no_cmo_emb" else e
    c_in = F.linear(torch.cat((cr, ce), dim=-1), _t(sd, "cmo_process.poseEmbedding.weight", dtype), _t(sd, "cmo_process.poseEmbedding.bias", dtype))
    xs = c_in + x_in
    if mutant != "no_pe":
        xs = xs + _t(sd, "sequence_pos_encoder.pe", dtype)[:T, 0][None]
    return xs


def stack_on(sd, cfg, xs, scan, dtype, mutant=None):
    """xs [B, T, d] sample-major -> the stack's output in the same layout."""
    if mutant == "other_axis":
        scan = "frames" if scan == "batch" else "batch"
    if scan == "batch":
        return gru_stack(sd, cfg, xs, dtype, mutant)                             # steps = samples, sequences = frames
    if scan == "frames":
        return gru_stack(sd, cfg, xs.transpose(0, 1), dtype, mutant).transpose(0, 1)
    raise ValueError(scan)


def _project(sd, out, shape, dtype):
    B, J, Fe, T = shape
    o = F.linear(out, _t(sd, "output_process.poseFinal.weight", dtype), _t(sd, "output_process.poseFinal.bias", dtype))
    return o.reshape(B, T, J, Fe).permute(0, 2, 3, 1)


def cmdm_forward(sd, cfg, x, timesteps, y, scan="batch", dtype=torch.float32, mutant=None):
    """x [B,J,F,T], timesteps [B] int64 (original indices), y dict -> x0_hat [B,J,F,T] in `dtype`."""
    if cfg["cm_mode"] != "add":
        raise NotImplementedError("arch='gru' is cm_mode='add' only (cmdm.py:244-247)")
    with torch.no_grad():
        xs = xseq_of(sd, cfg, x, timesteps, y, dtype, mutant)
        return _project(sd, stack_on(sd, cfg, xs, scan, dtype, mutant), x.shape, dtype)


def cfg_forward(sd, cfg, x, timesteps, y, scan="batch", dtype=torch.float32, mutant=None):
    """ClassifierFreeSampleModel.forward around the gru forward: two forwards of B rows each, so the batch scan restarts at the second."""
    with torch.no_grad():
        if mutant == "no_restart":                                               # one scan over the 2 B rows: the state runs on into the uncond half
            B = x.shape[0]
            xs = torch.cat((xseq_of(sd, cfg, x, timesteps, y, dtype), xseq_of(sd, cfg, x, timesteps, dict(y, uncond=True), dtype)))
            o = stack_on(sd, cfg, xs, scan, dtype)
            out, out_u = _project(sd, o[:B], x.shape, dtype), _project(sd, o[B:], x.shape, dtype)
        else:
            out = cmdm_forward(sd, cfg, x, timesteps, y, scan, dtype, mutant)
            out_u = cmdm_forward(sd, cfg, x, timesteps, dict(y, uncond=True), scan, dtype, mutant)
    return out_u + torch.as_tensor(y["scale"]).to(dtype).view(-1, 1, 1, 1) * (out - out_u)
