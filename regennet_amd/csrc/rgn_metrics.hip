// The metrics of the reference's unconstrained evaluation (eval/unconstrained/metrics/{kid,precision_recall}.py) on device features, without a
// kernel matrix or a distance matrix ever reaching memory.
//
//   k_poly_mmd_band   polynomial-kernel MMD over index-drawn subsets (kid.py:8-126). Workgroup (ti, q, s) owns the 64-row band ti of kernel matrix
//                     q (0: K_XX, 1: K_YY, 2: K_XY) of subset s and walks its 64-column tiles tj = 0, 1, ... in order. Rows and columns are gathered
//                     straight from X / Y through idx_x[s] / idx_y[s]. A tile's dot products run on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: exact
//                     fp32 products, fp32 accumulation over D in 32-deep chunks, columns past D zero-filled); then per entry, in fp32 without
//                     contraction, s = fl(fl(gamma dot) + coef0) and k = s^degree by degree - 1 multiplications (sklearn's polynomial_kernel on fp32
//                     inputs). Entries of rows or columns past m are set to 0.
//                     The tile goes to LDS as fp32 and is reduced in fp64, every sum in ONE fixed order: thread (r = t & 63, quarter = t >> 6) adds
//                     its 16 columns of row r ascending (value and square), the four quarters are added ascending, and the row's running sums take
//                     tile tj after tile tj - 1. K_XY's column sums are formed the same way over rows and leave the workgroup as one partial per
//                     (band, column): colpart[ti][j]. K_XX's / K_YY's diagonal comes out of tile tj == ti.
//                     Workspace of subset s, in doubles (mp = 64 ceil(m / 64), nt = mp / 64): rowsum[3][mp] | rowsq[3][mp] | diag[2][mp] |
//                     colpart[nt][mp]. Every entry the finisher reads is written by exactly one thread: nothing is zeroed, nothing is atomic.
//                     (K_XY's diagonal is read by the 'u-statistic' estimator only, which the reference never selects: it is not formed.)
//   k_poly_mmd_finish one workgroup per subset: the scalars of _mmd2_and_variance (kid.py:43-126) as 13 sums over i < m - thread t adds
//                     i = t, t + 256, ... ascending, then ONE thread per sum adds the 256 partials ascending (K_XY's column sums first take their nt
//                     band partials ascending) - and mmd2 ('unbiased') and var_est (var_at_m) evaluated in fp64 exactly as the reference writes them.
//
//   k_dist_tiles      the distances of precision_recall.py:30-53, direct-difference form: d2(a, b) = the fp32 chain acc = fma(t, t, acc), t = fl(a_c - b_c),
//                     over c = 0, 1, ..., D - 1 ascending from acc = 0 (one rounding per step; the zero-filled columns past D add exactly 0), and
//                     d = the correctly rounded fp32 square root of d2. Identical rows are at distance 0 exactly; no Gram form anywhere.
//                     A workgroup owns 64 rows and streams the 64-row column tiles through LDS in 32-deep chunks; thread (t >> 4, t & 15) holds the
//                     4 x 4 pairs (rows 4 (t >> 4) + 0..3, columns (t & 15) + 16 (0..3)).
//                       RADIUS: row i keeps the 16 smallest d2 over ALL columns j < N (j = i included, equal values kept separately) in one thread's
//                               registers, sorted; r_i = sqrt(the k-th of them, 0-based) - sqrt is monotone, so this is np.partition(d, k)[k].
//                       HITS:   flag_i = any_j (sqrt(d2(B_i, A_j)) <= r_j), the comparison in fp32.
//   k_count_flags     the count of the flags: one workgroup, integers, a second pass.
//
// Every store to global memory is an ordinary vector store from the C++ below; there is no floating-point atomic, so two calls on the same inputs
// agree bit for bit.
#include "rgn_device.h"

namespace rgn {

namespace {

constexpr int MT = 64;                 // rows / columns of a tile
constexpr int MK = 32;                 // depth of a staged chunk
constexpr int M_LD = MK + 4;           // LDS row of a staged chunk: 144 B, 16-B aligned quads, conflict-free ds_read_b128
constexpr int T_LD = MT + 1;           // LDS row of a result tile
constexpr int FIN_SUMS = 13;

// stage rows [row0, row0 + 64) x columns [k0, k0 + 32) of a gathered matrix: thread t takes row (t >> 3) + 32 i, quad t & 7
__device__ __forceinline__ void stage_chunk(float* dst, const float* __restrict__ src, const int* rows /*64 entries in LDS, -1: none*/, int D, int k0,
                                            int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (tid >> 3) + 32 * i, k = k0 + 4 * (tid & 7);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int g = rows[r];
        if (g >= 0 && k < D) v = *reinterpret_cast<const f32x4*>(src + (size_t)g * D + k);      // D % 4 == 0: a quad is inside the row or outside it
        *reinterpret_cast<f32x4*>(&dst[r * M_LD + 4 * (tid & 7)]) = v;
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_poly_mmd_band(const float* __restrict__ X, const float* __restrict__ Y, const int* __restrict__ idx_x,
                                                       const int* __restrict__ idx_y, int Nx, int Ny, int D, int m, int degree, float gamma,
                                                       float coef0, double* __restrict__ work) {
    __shared__ __attribute__((aligned(16))) float As[MT * M_LD];
    __shared__ __attribute__((aligned(16))) float Bs[MT * M_LD];
    __shared__ float Ts[MT * T_LD];
    __shared__ double red[3][4][MT];
    __shared__ int arow[MT], brow[MT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int ti = blockIdx.x, q = blockIdx.y, s = blockIdx.z;
    const int nt = gridDim.x, mp = nt * MT;
    const float* Am = q == 1 ? Y : X;
    const float* Bm = q == 0 ? X : Y;
    const int* ia = (q == 1 ? idx_y : idx_x) + (size_t)s * m;
    const int* ib = (q == 0 ? idx_x : idx_y) + (size_t)s * m;
    const int Na = q == 1 ? Ny : Nx, Nb = q == 0 ? Nx : Ny;
    double* ws = work + (size_t)s * (size_t)(8 + nt) * mp;
    double* rowsum = ws + (size_t)q * mp;
    double* rowsq = ws + (size_t)(3 + q) * mp;
    double* diag = ws + (size_t)(6 + (q & 1)) * mp;
    double* colpart = ws + (size_t)(8 + ti) * mp;

    if (tid < MT) {
        const int r = ti * MT + tid;
        int g = -1;
        if (r < m) {
            g = ia[r];
            g = g < 0 || g >= Na ? 0 : g;         // an index outside the set (the caller's error): an unspecified result, never an access outside X / Y
        }
        arow[tid] = g;
    }
    double run_sum = 0.0, run_sq = 0.0;            // threads 0..63: row ti * 64 + tid over the tiles walked so far

    for (int tj = 0; tj < nt; ++tj) {
        if (tid < MT) {
            const int c = tj * MT + tid;
            int g = -1;
            if (c < m) {
                g = ib[c];
                g = g < 0 || g >= Nb ? 0 : g;
            }
            brow[tid] = g;
        }
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int k0 = 0; k0 < D; k0 += MK) {
            __syncthreads();                       // the previous chunk's operands (and, at k0 == 0, the previous tile's Ts / red / brow readers) are done
            stage_chunk(As, Am, arow, D, k0, tid);
            stage_chunk(Bs, Bm, brow, D, k0, tid);
            __syncthreads();
#pragma unroll
            for (int kc = 0; kc < MK; kc += 8) {
                // operand layout of the 32x32x2 fp32 MFMA: lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31]; the quad read
                // here feeds four instructions, instruction j taking k = kc + 4 (l >> 5) + j on both sides
                const f32x4 a = *reinterpret_cast<const f32x4*>(&As[(wm * 32 + (lane & 31)) * M_LD + kc + 4 * (lane >> 5)]);
                const f32x4 b = *reinterpret_cast<const f32x4*>(&Bs[(wn * 32 + (lane & 31)) * M_LD + kc + 4 * (lane >> 5)]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
            }
        }
        // C/D layout: column = lane & 31, row = mfma32_row(i, lane >> 5)
        {
            const int c = wn * 32 + (lane & 31);
            const bool cin = tj * MT + c < m;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = wm * 32 + mfma32_row(i, lane >> 5);
                const float sv = __fadd_rn(__fmul_rn(gamma, acc[i]), coef0);
                float kv = sv;
                for (int p = 1; p < degree; ++p) kv = __fmul_rn(kv, sv);
                Ts[r * T_LD + c] = (cin && ti * MT + r < m) ? kv : 0.f;
            }
        }
        __syncthreads();
        {
            const int r = tid & 63, qd = tid >> 6;
            double p = 0.0, p2 = 0.0;
            for (int c = 16 * qd; c < 16 * qd + 16; ++c) {
                const double v = Ts[r * T_LD + c];
                p += v;
                p2 += v * v;
            }
            red[0][qd][r] = p;
            red[1][qd][r] = p2;
            if (q == 2) {
                double pc = 0.0;
                for (int rr = 16 * qd; rr < 16 * qd + 16; ++rr) pc += (double)Ts[rr * T_LD + r];
                red[2][qd][r] = pc;
            }
        }
        __syncthreads();
        if (tid < MT) {
            run_sum += ((red[0][0][tid] + red[0][1][tid]) + red[0][2][tid]) + red[0][3][tid];
            run_sq += ((red[1][0][tid] + red[1][1][tid]) + red[1][2][tid]) + red[1][3][tid];
            if (q < 2 && tj == ti) diag[ti * MT + tid] = (double)Ts[tid * T_LD + tid];
        } else if (tid < 2 * MT && q == 2) {
            const int c = tid - MT;
            colpart[tj * MT + c] = ((red[2][0][c] + red[2][1][c]) + red[2][2][c]) + red[2][3][c];
        }
    }
    if (tid < MT) {
        rowsum[ti * MT + tid] = run_sum;
        rowsq[ti * MT + tid] = run_sq;
    }
}

__global__ __launch_bounds__(256) void k_poly_mmd_finish(const double* __restrict__ work, int m, int nt, int var_at_m, double* __restrict__ mmds,
                                                         double* __restrict__ vars) {
    __shared__ double part[FIN_SUMS][256];
    __shared__ double tot[FIN_SUMS];
    const int tid = threadIdx.x, s = blockIdx.x, mp = nt * MT;
    const double* ws = work + (size_t)s * (size_t)(8 + nt) * mp;
    double a[FIN_SUMS];
#pragma unroll
    for (int k = 0; k < FIN_SUMS; ++k) a[k] = 0.0;
    for (int i = tid; i < m; i += 256) {
        const double dx = ws[6 * (size_t)mp + i], dy = ws[7 * (size_t)mp + i];
        const double kx = ws[i] - dx, ky = ws[(size_t)mp + i];                 // Kt_XX_sums[i]; K_YY.sum(axis=1)[i]
        const double kty = ky - dy, xy1 = ws[2 * (size_t)mp + i];               // Kt_YY_sums[i]; K_XY_sums_1[i]
        double xy0 = 0.0;                                                       // K_XY_sums_0[i]
        for (int t = 0; t < nt; ++t) xy0 += ws[(size_t)(8 + t) * mp + i];
        a[0] += dx * dx;                        // sum_diag2_X
        a[1] += dy * dy;                        // sum_diag2_Y
        a[2] += kx;                             // Kt_XX_sum
        a[3] += kty;                            // Kt_YY_sum
        a[4] += xy0;                            // K_XY_sum
        a[5] += ws[3 * (size_t)mp + i];         // _sqn(K_XX)
        a[6] += ws[4 * (size_t)mp + i];         // _sqn(K_YY)
        a[7] += ws[5 * (size_t)mp + i];         // _sqn(K_XY)
        a[8] += kx * xy1;                       // dot_XX_XY
        a[9] += kty * xy0;                      // dot_YY_YX
        a[10] += kx * kx;                       // _sqn(Kt_XX_sums)
        a[11] += kty * kty;                     // _sqn(Kt_YY_sums)
        a[12] += xy1 * xy1 + xy0 * xy0;         // _sqn(K_XY_sums_1) + _sqn(K_XY_sums_0)
    }
#pragma unroll
    for (int k = 0; k < FIN_SUMS; ++k) part[k][tid] = a[k];
    __syncthreads();
    if (tid < FIN_SUMS) {
        double v = 0.0;
        for (int t = 0; t < 256; ++t) v += part[tid][t];
        tot[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        const double md = (double)m, m1 = md - 1.0, m2 = md - 2.0, vm = (double)var_at_m;
        const double Kt_XX_sum = tot[2], Kt_YY_sum = tot[3], K_XY_sum = tot[4];
        const double Kt_XX_2_sum = tot[5] - tot[0], Kt_YY_2_sum = tot[6] - tot[1], K_XY_2_sum = tot[7];
        const double dots = tot[8] + tot[9];
        const double mmd2 = (Kt_XX_sum + Kt_YY_sum) / (md * m1) - 2.0 * K_XY_sum / (md * md);
        const double sq2 = Kt_XX_sum * Kt_XX_sum + Kt_YY_sum * Kt_YY_sum, mm1 = (md * m1) * (md * m1), m4 = md * md * md * md;
        const double zeta1 = 1.0 / (md * m1 * m2) * (tot[10] - Kt_XX_2_sum + tot[11] - Kt_YY_2_sum) - 1.0 / mm1 * sq2 +
                             1.0 / (md * md * m1) * (tot[12] - 2.0 * K_XY_2_sum) - 2.0 / m4 * (K_XY_sum * K_XY_sum) - 2.0 / (md * md * m1) * dots +
                             2.0 / (md * md * md * m1) * (Kt_XX_sum + Kt_YY_sum) * K_XY_sum;
        const double zeta2 = 1.0 / (md * m1) * (Kt_XX_2_sum + Kt_YY_2_sum) - 1.0 / mm1 * sq2 + 2.0 / (md * md) * K_XY_2_sum -
                             2.0 / m4 * (K_XY_sum * K_XY_sum) - 4.0 / (md * md * m1) * dots +
                             4.0 / (md * md * md * m1) * (Kt_XX_sum + Kt_YY_sum) * K_XY_sum;
        mmds[s] = mmd2;
        vars[s] = 4.0 * (vm - 2.0) / (vm * (vm - 1.0)) * zeta1 + 2.0 / (vm * (vm - 1.0)) * zeta2;
    }
}

// RADIUS: rows and columns are both A (M == N), out_r[i] = the k-th smallest distance of row i. HITS: rows are B [M, D], columns A [N, D] with their
// radii, flags[i] = any column within its radius.
template <bool HITS>
__global__ __launch_bounds__(256) void k_dist_tiles(const float* __restrict__ R, const float* __restrict__ A, const float* __restrict__ radii, int M,
                                                    int N, int D, int k, float* __restrict__ out_r, uint8_t* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) float Qs[MT * M_LD];
    __shared__ __attribute__((aligned(16))) float Cs[MT * M_LD];
    __shared__ float Ts[HITS ? 1 : MT * T_LD];
    __shared__ float rad[MT];
    __shared__ int hit[MT];
    __shared__ int qrow[MT], crow[MT];

    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const int row0 = blockIdx.x * MT;
    if (tid < MT) {
        qrow[tid] = row0 + tid < M ? row0 + tid : -1;
        hit[tid] = 0;
    }
    float best[16];                                // threads 0..63 (RADIUS): the 16 smallest d2 of row row0 + tid so far, ascending
#pragma unroll
    for (int i = 0; i < 16; ++i) best[i] = INFINITY;

    for (int col0 = 0; col0 < N; col0 += MT) {
        __syncthreads();                           // the previous tile's readers of rad (HITS) are done
        if (tid < MT) {
            const int c = col0 + tid;
            crow[tid] = c < N ? c : -1;
            if (HITS) rad[tid] = c < N ? radii[c] : 0.f;
        }
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
        for (int k0 = 0; k0 < D; k0 += MK) {
            __syncthreads();
            stage_chunk(Qs, R, qrow, D, k0, tid);
            stage_chunk(Cs, A, crow, D, k0, tid);
            __syncthreads();
#pragma unroll 2
            for (int c = 0; c < MK; c += 4) {          // quads of the chunk (ds_read_b128); inside a quad and across quads c ascends: the chain's order
                f32x4 qv[4], cv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) qv[i] = *reinterpret_cast<const f32x4*>(&Qs[(4 * tr + i) * M_LD + c]);
#pragma unroll
                for (int j = 0; j < 4; ++j) cv[j] = *reinterpret_cast<const f32x4*>(&Cs[(tc + 16 * j) * M_LD + c]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float t = __fsub_rn(qv[i][e], cv[j][e]);
                            acc[i][j] = __fmaf_rn(t, t, acc[i][j]);
                        }
            }
        }
        if (HITS) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = tc + 16 * j;
                if (col0 + c < N) {
                    const float rj = rad[c];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (__fsqrt_rn(acc[i][j]) <= rj) hit[4 * tr + i] = 1;      // (every writer stores the same 1)
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = tc + 16 * j;
                    Ts[(4 * tr + i) * T_LD + c] = col0 + c < N ? acc[i][j] : INFINITY;
                }
            __syncthreads();
            if (tid < MT) {
                for (int c = 0; c < MT; ++c) {
                    const float v = Ts[tid * T_LD + c];
                    if (v < best[15]) {
                        best[15] = v;
#pragma unroll
                        for (int i = 15; i > 0; --i) {
                            const float lo = fminf(best[i - 1], best[i]), hi = fmaxf(best[i - 1], best[i]);
                            best[i - 1] = lo;
                            best[i] = hi;
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    if (tid < MT && row0 + tid < M) {
        if (HITS) {
            flags[row0 + tid] = (uint8_t)hit[tid];
        } else {
            float v = best[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) v = i == k ? best[i] : v;
            out_r[row0 + tid] = __fsqrt_rn(v);
        }
    }
}

__global__ __launch_bounds__(256) void k_count_flags(const uint8_t* __restrict__ flags, int M, int* __restrict__ count) {
    __shared__ int part[256];
    int n = 0;
    for (int i = threadIdx.x; i < M; i += 256) n += flags[i] != 0;
    part[threadIdx.x] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < 256; ++i) t += part[i];
        *count = t;
    }
}

unsigned long long poly_mmd_workspace_bytes(int S, int m) {
    const unsigned long long nt = ((unsigned long long)m + MT - 1) / MT, mp = nt * MT;
    return (unsigned long long)S * (8 + nt) * mp * sizeof(double);
}

hipError_t launch_poly_mmd(const float* X, const float* Y, const int* idx_x, const int* idx_y, int Nx, int Ny, int D, int S, int m, int degree,
                           float gamma, float coef0, double* work, double* mmds, double* vars, hipStream_t s) {
    const int nt = (m + MT - 1) / MT;
    hipLaunchKernelGGL(k_poly_mmd_band, dim3((unsigned)nt, 3, (unsigned)S), dim3(256), 0, s, X, Y, idx_x, idx_y, Nx, Ny, D, m, degree, gamma, coef0, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_poly_mmd_finish, dim3((unsigned)S), dim3(256), 0, s, work, m, nt, Nx < Ny ? Nx : Ny, mmds, vars);
    return hipGetLastError();
}

hipError_t launch_knn_radius(const float* A, int N, int D, int k, float* radii, hipStream_t s) {
    hipLaunchKernelGGL(k_dist_tiles<false>, dim3((unsigned)((N + MT - 1) / MT)), dim3(256), 0, s, A, A, (const float*)nullptr, N, N, D, k, radii,
                       (uint8_t*)nullptr);
    return hipGetLastError();
}

hipError_t launch_manifold_hits(const float* B, const float* A, const float* radii, int M, int N, int D, uint8_t* flags, int* count, hipStream_t s) {
    hipLaunchKernelGGL(k_dist_tiles<true>, dim3((unsigned)((M + MT - 1) / MT)), dim3(256), 0, s, B, A, radii, M, N, D, 0, (float*)nullptr, flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_count_flags, dim3(1), dim3(256), 0, s, flags, M, count);
    return hipGetLastError();
}

}  // namespace rgn
