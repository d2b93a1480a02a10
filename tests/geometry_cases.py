"""The model geometries tests/test_geometry_gpu.py runs on the GPU, as `synth.get_config("ntu_action", **over)` overrides, shared with the CPU
checks of rgn_create (tests/test_abi_cpu.py) - every one of them must pass the argument checks that run before the device is touched.
Also the two tile constants the short-sequence cases are derived from, pinned to the kernel sources by tests/test_host_logic_cpu.py."""

M2_NSAMP = 4   # rgn_mlp2.hip  M2::NSAMP: samples a 64-row tile of k_mlp2 may touch    -> mlp_supported:    63 / Tq + 2 <= NSAMP
MX_NSAMP = 2   # rgn_mlp_x3.hip MX::NSAMP: samples a 32-row tile of k_mlp_x3 may touch -> mlp_x3_supported: 31 / Tq + 2 <= NSAMP


def first_tq(rows, nsamp):
    """Smallest Tq with (rows - 1) / Tq + 2 <= nsamp (integer division): the short side of the predicate is Tq - 1."""
    return next(tq for tq in range(1, rows + 1) if (rows - 1) // tq + 2 <= nsamp)


TQ_MLP = first_tq(64, M2_NSAMP)      # 22: k_mlp2 from 22 tokens on, k_rowgemm<LN> at 21
TQ_MLP_X3 = first_tq(32, MX_NSAMP)   # 32: k_mlp_x3 from 32 tokens on, k_gemm_x3 + k_layernorm at 31

HEADS_FUSED = [dict(latent_dim=128, num_heads=1), dict(latent_dim=256, num_heads=2), dict(latent_dim=1024, num_heads=8)]
HEADS_D512 = [dict(num_heads=8), dict(num_heads=16), dict(num_heads=32)]
PLAIN_ATTN = [dict(num_heads=64), dict(latent_dim=64, num_heads=8, ff_size=128)]
FF_WIDTHS = [dict(ff_size=32), dict(ff_size=96), dict(ff_size=100), dict(ff_size=384), dict(ff_size=1000), dict(ff_size=1056),
             dict(latent_dim=64, ff_size=100)]
F_STEP = [dict(njoints=54, nfeats=6), dict(njoints=85, nfeats=4), dict(njoints=58, nfeats=6), dict(njoints=88, nfeats=4)]          # F = 324, 340, 348, 352
F_OFF_STEP = [dict(njoints=80, nfeats=4), dict(njoints=89, nfeats=4), dict(njoints=8, nfeats=4), dict(njoints=33, nfeats=1),
              dict(njoints=263, nfeats=1), dict(njoints=1, nfeats=1)]                                                             # F = 320, 356, 32, 33, 263, 1
SHORT_T = sorted({1, 2, 7, 8, TQ_MLP - 1, TQ_MLP, TQ_MLP_X3 - 1, TQ_MLP_X3})
CONDITIONING = [dict(cond_mode="text", clip_dim=100), dict(cond_mode="text", clip_dim=768), dict(num_actions=1)]
DEPTH = [dict(layers=9)]

ACCEPTED = (HEADS_FUSED + HEADS_D512 + PLAIN_ATTN + [dict(g, num_frames=200) for g in PLAIN_ATTN] + [dict(g, num_frames=160, emb_trans_dec=True) for g in PLAIN_ATTN] +
            FF_WIDTHS + F_STEP + F_OFF_STEP + [dict(num_frames=t) for t in SHORT_T] + CONDITIONING + DEPTH)
