// Vision Mamba backbone (pose/vim/models_mamba.py:VisionMamba with the bidirectional "v2" mixer of the Vim paper) for gfx950,
// wave64.  The dense Linears (patch embedding, in_proj, x_proj, out_proj, head) run on the existing GEMMs; this file holds the
// rest, all fp32:
//   patch_gather     NCHW image -> [B g g, 768] operand rows of the overlapping 16 x 16 patches (fp32 or activation planes)
//   place_tokens     patch rows + the class token at row M / 2, + pos_embed -> the token matrix [B, L, D]
//   add_rmsnorm      r = hidden + residual, y = r rsqrt(mean r^2 + eps) w -> fp32 residual and the in_proj operand; a wave per row
//   conv1d_silu      depthwise width-4 convolution + SiLU, causal (forward direction) and anti-causal (backward direction, in
//                    un-reversed time) in one launch, x read in place from xz
//   scan_state / scan_out   the selective scan of both directions of a layer (DESIGN.md "Vision Mamba"):
//       h_t = exp(delta_t A) h_{t-1} + (delta_t x_t) B_t,  y_t = <C_t, h_t> + D x_t,  delta_t = softplus(dt_proj(dt_t))
//     is a first-order linear recurrence, so the sequence is cut into chunks of SCAN_T steps.  scan_state runs every chunk from
//     h = 0 and keeps its end state and its sum of delta (the chunk's decay is exp(A sum delta)); scan_out rebuilds a chunk's
//     start state from the chunks before it IN CHUNK ORDER, re-runs the chunk and writes (y_fwd silu(z) + y_bwd silu(z)) / 2.
//     Nothing depends on the grid or on B.  A workgroup = one chunk x 16 channels x both directions (waves 0-3 walk time
//     upwards, waves 4-7 downwards); the 16 states of a channel are 16 adjacent lanes (one DPP row), <C_t, h_t> a row
//     reduction by four row rotations; dt | B | C of the chunk are staged in LDS once for the 16 channels.  The loop is bound by
//     vector issue, not memory (profiles/vim.md): what it reads per step is two LDS pairs, what it keeps is in registers.
#include "common.h"
#include "kernels.h"
#include "linear.h"

namespace {

constexpr int NS = 16;          // d_state
constexpr int SCAN_T = 64;      // time steps per chunk
constexpr int SCAN_CH = 16;     // channels per workgroup and direction
constexpr int XS_MAX = 64;      // R + 2 NS <= 64

__device__ __forceinline__ float silu(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float softplus(float v) { return v > 20.0f ? v : log1pf(expf(v)); }   // F.softplus: beta 1, threshold 20

// sum over the 16 lanes of a DPP row, the same bits in every lane (a symmetric tree of commutative adds)
template <int CTRL>
__device__ __forceinline__ float row_ror(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row_sum16(float v) {
    v += row_ror<0x128>(v);
    v += row_ror<0x124>(v);
    v += row_ror<0x122>(v);
    v += row_ror<0x121>(v);
    return v;
}

// image [B, 3, S, S] -> rows [B g g, 768], columns (channel, kh, kw): one thread per 16-byte quad of a row
template <bool PLANES>
__global__ __launch_bounds__(256) void patch_gather_kernel(const float* __restrict__ img, void* out, int S, int g, int stride, long long quads,
                                                           unsigned* flag) {
    pope_range_acc acc;
    for (long long q = blockIdx.x * 256ll + threadIdx.x; q < quads; q += 256ll * gridDim.x) {
        const int col = int(q % 192) * 4;
        const long long row = q / 192;
        const int gx = int(row % g), gy = int((row / g) % g);
        const long long b = row / (1ll * g * g);
        const int c = col >> 8, kh = (col >> 4) & 15, kw = col & 15;
        const f32x4 v = *reinterpret_cast<const f32x4*>(img + ((b * 3 + c) * S + gy * stride + kh) * S + gx * stride + kw);
        if constexpr (PLANES) {
            const f32x4 sc = v * K_PLANES_ACT_SCALE;
            acc.add(sc);
            pope_planes_store(static_cast<_Float16*>(out) + row * 2 * 768, col, sc);
        } else {
            *reinterpret_cast<f32x4*>(static_cast<float*>(out) + row * 768 + col) = v;
        }
    }
    if constexpr (PLANES) pope_range_flag(flag, POPE_RANGE_PATCH, acc.bad());
}

// tokens [B, L, D]: row l of an image = (l == mid ? cls : patch row l - (l > mid)) + pos[l]
__global__ __launch_bounds__(256) void place_tokens_kernel(const float* __restrict__ pe, const float* __restrict__ cls, const float* __restrict__ pos,
                                                           float* __restrict__ tok, int L, int D, int mid, long long quads) {
    const int dq = D >> 2;
    for (long long q = blockIdx.x * 256ll + threadIdx.x; q < quads; q += 256ll * gridDim.x) {
        const int c = int(q % dq) * 4;
        const long long row = q / dq;
        const int l = int(row % L);
        const long long b = row / L;
        const f32x4 v = l == mid ? *reinterpret_cast<const f32x4*>(cls + c)
                                 : *reinterpret_cast<const f32x4*>(pe + (b * (L - 1) + (l > mid ? l - 1 : l)) * D + c);
        *reinterpret_cast<f32x4*>(tok + 4 * q) = v + *reinterpret_cast<const f32x4*>(pos + size_t(l) * D + c);
    }
}

// a wave per row; the row is read twice (the second time from L1 / L2) so that any D % 4 == 0 fits
template <bool PLANES>
__global__ __launch_bounds__(256) void add_rmsnorm_kernel(const float* hidden, const float* res_in, float* res_out, const float* __restrict__ w,
                                                          void* y, long long rows, int D, float eps, long long rs, long long r0, unsigned* flag) {
    const int lane = threadIdx.x & 63;
    const long long r = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (r >= rows) return;
    const long long in = (r * rs + r0) * D;
    float s = 0.f;
    for (int c = 4 * lane; c < D; c += 256) {
        f32x4 v = *reinterpret_cast<const f32x4*>(hidden + in + c);
        if (res_in) v = v + *reinterpret_cast<const f32x4*>(res_in + in + c);
        s += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(s) / float(D) + eps);
    pope_range_acc acc;
    for (int c = 4 * lane; c < D; c += 256) {
        f32x4 v = *reinterpret_cast<const f32x4*>(hidden + in + c);
        if (res_in) v = v + *reinterpret_cast<const f32x4*>(res_in + in + c);
        if (res_out) *reinterpret_cast<f32x4*>(res_out + in + c) = v;   // res_out may be res_in: the lane's own quad, read above
        const f32x4 o = (v * rstd) * *reinterpret_cast<const f32x4*>(w + c);
        if constexpr (PLANES) {
            const f32x4 sc = o * K_PLANES_ACT_SCALE;
            acc.add(sc);
            pope_planes_store(static_cast<_Float16*>(y) + r * 2 * D, c, sc);
        } else {
            *reinterpret_cast<f32x4*>(static_cast<float*>(y) + r * D + c) = o;
        }
    }
    if constexpr (PLANES) pope_range_flag(flag, POPE_RANGE_LAYERNORM, acc.bad());
}

struct DirPtrs { const float *conv_w, *conv_b, *dt_w, *dt_b, *A_log, *D; };
struct DirPair { DirPtrs d[2]; };

// xc[0][row t] = silu(b + sum_k w[k] x[t - 3 + k]), xc[1][row t] = silu(b' + sum_k w'[k] x[t + 3 - k]); rows outside [0, L) are zero.
// One thread per (direction, row, channel quad).
__global__ __launch_bounds__(256) void conv1d_silu_kernel(const float* __restrict__ x, int ldx, DirPair p, int L, int E, long long M,
                                                          float* __restrict__ xc, long long quads) {
    const int eq = E >> 2;
    for (long long q = blockIdx.x * 256ll + threadIdx.x; q < quads; q += 256ll * gridDim.x) {
        const int e = int(q % eq) * 4;
        const long long rr = q / eq;
        const int dir = rr >= M;
        const long long row = rr - (dir ? M : 0);
        const int t = int(row % L);
        const DirPtrs& w = p.d[dir];
        f32x4 wk[4];   // wk[j][k]: tap k of channel e + j
#pragma unroll
        for (int j = 0; j < 4; ++j) wk[j] = *reinterpret_cast<const f32x4*>(w.conv_w + size_t(e + j) * 4);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int off = dir ? 3 - k : k - 3;
            if (t + off < 0 || t + off >= L) continue;
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + (row + off) * ldx + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(wk[j][k], v[j], acc[j]);
        }
        acc = acc + *reinterpret_cast<const f32x4*>(w.conv_b + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = silu(acc[j]);
        *reinterpret_cast<f32x4*>(xc + rr * E + e) = acc;
    }
}

// LDS of one direction of a scan workgroup: the chunk's x_proj rows, (delta, delta x) and x of its 16 channels, and y — whose space
// holds the 16 dt_proj rows until delta is computed.  2 x 32 KB: two workgroups per CU.
struct ScanLds {
    float xd[SCAN_T * XS_MAX];
    f32x2 dd[SCAN_T * SCAN_CH];
    float ux[SCAN_T * SCAN_CH];
    float y[SCAN_T * SCAN_CH];
};
static_assert(SCAN_CH * 33 <= SCAN_T * SCAN_CH && 2 * sizeof(ScanLds) <= 65536, "scan LDS");
constexpr float LOG2E = 1.44269504088896340736f;

// Stages chunk rows [row0, row0 + len) for the 256 threads `tid` of one direction and computes delta; ends with a workgroup barrier.
__device__ __forceinline__ void scan_stage(ScanLds& s, const float* __restrict__ xc, const float* __restrict__ xdbl, const DirPtrs& w, int tid,
                                          long long row0, int len, int E, int R, int e0) {
    const int XS = R + 2 * NS;
    float* wl = s.y;
    {   // the chunk's rows of xdbl are contiguous: len * XS floats, XS % 4 == 0; in LDS a row has the fixed pitch XS_MAX
        const f32x4* src = reinterpret_cast<const f32x4*>(xdbl + row0 * XS);
        const int xq = XS >> 2;
        for (int i = tid; i < len * xq; i += 256) reinterpret_cast<f32x4*>(s.xd)[(i / xq) * (XS_MAX / 4) + i % xq] = src[i];
    }
    const int ch = tid & 15;
    for (int t = tid >> 4; t < len; t += 16) s.ux[t * SCAN_CH + ch] = xc[(row0 + t) * E + e0 + ch];
    for (int i = tid; i < SCAN_CH * R; i += 256) wl[(i / R) * 33 + i % R] = w.dt_w[size_t(e0) * R + i];
    __syncthreads();
    const float bias = w.dt_b[e0 + ch];
    for (int t = tid >> 4; t < len; t += 16) {
        float a = 0.f;
        for (int r = 0; r < R; ++r) a = fmaf(wl[ch * 33 + r], s.xd[t * XS_MAX + r], a);
        const float dlt = softplus(a + bias);
        s.dd[t * SCAN_CH + ch] = f32x2{dlt, dlt * s.ux[t * SCAN_CH + ch]};
    }
    __syncthreads();
}

// One step of lane (channel ch, state n) at chunk row t: h <- exp(delta A) h + (delta x) B_t[n]; the decay as
// exp2((delta A) log2 e) on the hardware exponential, which underflows to 0 and never leaves [0, 1].  bc = the row's B_t[n]; C_t[n] is NS on.
__device__ __forceinline__ void scan_step(const f32x2 d, const float* bc, float A, float& h) {
    h = fmaf(__builtin_amdgcn_exp2f((d[0] * A) * LOG2E), h, d[1] * bc[0]);
}

// pass 1: the end state of every chunk run from h = 0 and its sum of delta.  hloc [2, B, nch, E, 16], dsum [2, B, nch, E]
__global__ __launch_bounds__(512) void scan_state_kernel(const float* __restrict__ xc, const float* __restrict__ xdbl, DirPair p, int L, int E, int R,
                                                         long long M, int nch, float* __restrict__ hloc, float* __restrict__ dsum) {
    __shared__ ScanLds lds[2];
    const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8), tid = threadIdx.x & 255;   // wave-uniform: scalar addressing
    const int chunk = blockIdx.x, e0 = blockIdx.y * SCAN_CH, b = blockIdx.z, B = gridDim.z;
    const int t0 = chunk * SCAN_T, len = min(SCAN_T, L - t0);
    const DirPtrs& w = p.d[dir];
    ScanLds& s = lds[dir];
    constexpr int XS = XS_MAX;   // LDS pitch of a staged x_proj row
    scan_stage(s, xc + dir * M * E, xdbl + dir * M * (R + 2 * NS), w, tid, 1ll * b * L + t0, len, E, R, e0);
    if (chunk == (dir ? 0 : nch - 1)) return;   // the direction's last chunk: nothing comes after it
    const int n = tid & 15, ch = tid >> 4, e = e0 + ch;
    const float A = -expf(w.A_log[size_t(e) * NS + n]);
    const int step = dir ? -1 : 1;
    const f32x2* dd = s.dd + (dir ? len - 1 : 0) * SCAN_CH + ch;
    const float* bc = s.xd + (dir ? len - 1 : 0) * XS + R + n;
    float h = 0.f, sum = 0.f;
#pragma unroll 4
    for (int i = 0; i < len; ++i) {
        const f32x2 d = dd[i * step * SCAN_CH];
        scan_step(d, bc + i * step * XS, A, h);
        sum += d[0];
    }
    const size_t slot = (size_t(dir) * B + b) * nch + chunk;
    hloc[(slot * E + e) * NS + n] = h;
    if (n == 0) dsum[slot * E + e] = sum;
}

// pass 2: start state from the chunks before this one in the direction's order, the chunk again, the gated mean of the two directions
template <bool PLANES>
__global__ __launch_bounds__(512) void scan_out_kernel(const float* __restrict__ xc, const float* __restrict__ z, int ldz,
                                                       const float* __restrict__ xdbl, DirPair p, int L, int E, int R, long long M, int nch,
                                                       const float* __restrict__ hloc, const float* __restrict__ dsum, void* out, unsigned* flag) {
    __shared__ ScanLds lds[2];
    const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8), tid = threadIdx.x & 255;   // wave-uniform: scalar addressing
    const int chunk = blockIdx.x, e0 = blockIdx.y * SCAN_CH, b = blockIdx.z, B = gridDim.z;
    const int t0 = chunk * SCAN_T, len = min(SCAN_T, L - t0);
    const DirPtrs& w = p.d[dir];
    ScanLds& s = lds[dir];
    constexpr int XS = XS_MAX;   // LDS pitch of a staged x_proj row
    scan_stage(s, xc + dir * M * E, xdbl + dir * M * (R + 2 * NS), w, tid, 1ll * b * L + t0, len, E, R, e0);
    const int n = tid & 15, ch = tid >> 4, e = e0 + ch;
    const float A = -expf(w.A_log[size_t(e) * NS + n]);
    float h = 0.f;
    {   // the carry, chunk by chunk in the direction's order: forward 0 .. chunk - 1, backward nch - 1 .. chunk + 1
        const size_t base = (size_t(dir) * B + b) * nch;
        const int steps = dir ? nch - 1 - chunk : chunk;
        for (int j = 0; j < steps; ++j) {
            const size_t slot = base + (dir ? nch - 1 - j : j);
            h = fmaf(__builtin_amdgcn_exp2f((dsum[slot * E + e] * A) * LOG2E), h, hloc[(slot * E + e) * NS + n]);
        }
    }
    // steps in blocks of 16: lane n keeps <C, h> of the block's step n (every lane of the row holds every sum) and stores it once
    const int step = dir ? -1 : 1, first = dir ? len - 1 : 0;
    const f32x2* dd = s.dd + first * SCAN_CH + ch;
    const float* bc = s.xd + first * XS + R + n;
    float* yo = s.y + first * SCAN_CH + ch;
    for (int ib = 0; ib < len; ib += 16) {
        float keep = 0.f;
        if (len - ib >= 16) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int o = (ib + j) * step;
                scan_step(dd[o * SCAN_CH], bc + o * XS, A, h);
                const float y = row_sum16(bc[o * XS + NS] * h);
                keep = j == n ? y : keep;
            }
        } else {
            for (int j = 0; j < len - ib; ++j) {
                const int o = (ib + j) * step;
                scan_step(dd[o * SCAN_CH], bc + o * XS, A, h);
                const float y = row_sum16(bc[o * XS + NS] * h);
                keep = j == n ? y : keep;
            }
        }
        if (ib + n < len) yo[(ib + n) * step * SCAN_CH] = keep;
    }
    __syncthreads();
    // 64 steps x 16 channels = 256 quads: the first 256 threads write them, four lanes (64 bytes) per time step
    pope_range_acc acc;
    if (threadIdx.x < 256) {
        const int t = threadIdx.x >> 2, c4 = (threadIdx.x & 3) * 4;
        if (t < len) {
            const long long row = 1ll * b * L + t0 + t;
            const f32x4 zz = *reinterpret_cast<const f32x4*>(z + row * ldz + e0 + c4);
            const f32x4 yf = *reinterpret_cast<const f32x4*>(&lds[0].y[t * SCAN_CH + c4]) +
                             *reinterpret_cast<const f32x4*>(p.d[0].D + e0 + c4) * *reinterpret_cast<const f32x4*>(&lds[0].ux[t * SCAN_CH + c4]);
            const f32x4 yb = *reinterpret_cast<const f32x4*>(&lds[1].y[t * SCAN_CH + c4]) +
                             *reinterpret_cast<const f32x4*>(p.d[1].D + e0 + c4) * *reinterpret_cast<const f32x4*>(&lds[1].ux[t * SCAN_CH + c4]);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float g = silu(zz[j]);
                o[j] = (yf[j] * g + yb[j] * g) * 0.5f;
            }
            if constexpr (PLANES) {
                const f32x4 sc = o * K_PLANES_ACT_SCALE;
                acc.add(sc);
                pope_planes_store(static_cast<_Float16*>(out) + row * 2 * E, e0 + c4, sc);
            } else {
                *reinterpret_cast<f32x4*>(static_cast<float*>(out) + row * E + e0 + c4) = o;
            }
        }
    }
    if constexpr (PLANES) pope_range_flag(flag, POPE_RANGE_GELU, acc.bad());
}

// ---- host -----------------------------------------------------------------------------------------------------------------

DirPair dir_pair(const pope_vim_dir_weights* d) {
    DirPair p;
    for (int i = 0; i < 2; ++i) p.d[i] = DirPtrs{d[i].conv_w, d[i].conv_b, d[i].dt_w, d[i].dt_b, d[i].A_log, d[i].D};
    return p;
}

struct Geo { int g, L, mid, D, E, R, XS; long long M, P; };

bool geometry(const pope_vim_weights* w, int B, Geo& q) {
    if (!w || B <= 0 || B > 65535) return false;
    if (w->img < 16 || (w->img & 7) || (w->stride != 8 && w->stride != 16) || w->depth <= 0 || !w->layers_host) return false;
    if (w->dim < 64 || (w->dim & 63) || w->dim > 512 || !(w->eps > 0.f)) return false;
    q.g = (w->img - 16) / w->stride + 1;
    q.L = q.g * q.g + 1;
    q.mid = (q.g * q.g) / 2;
    q.D = w->dim; q.E = 2 * q.D; q.R = (q.D + 15) / 16; q.XS = q.R + 2 * NS;
    q.M = 1ll * B * q.L; q.P = 1ll * B * q.g * q.g;
    // the GEMMs address their rows through 32-bit byte offsets (gemm_planes.hip args_ok)
    return size_t(q.M + 256) * size_t(2 * q.E) * 4 < (size_t(1) << 32) - 512 && size_t(q.P + 256) * 768 * 4 < (size_t(1) << 32) - 512;
}

struct Layout { size_t hid, res, op, xz, xc, xdbl, so, scan, pa, pe, feat, total; };

Layout layout(const Geo& q, int B) {
    Layout l;
    l.hid = l.res = l.op = pope_align256(size_t(q.M) * q.D * 4);
    l.xz = pope_align256(size_t(q.M) * 2 * q.E * 4);
    l.xc = pope_align256(size_t(q.M) * 2 * q.E * 4);
    l.xdbl = pope_align256(size_t(q.M) * 2 * q.XS * 4);
    l.so = pope_align256(size_t(q.M) * q.E * 4);
    l.scan = pope_vim_scan_workspace(B, q.L, q.E);
    l.pa = pope_align256(size_t(q.P) * 768 * 4);
    l.pe = pope_align256(size_t(q.P) * q.D * 4);
    l.feat = pope_align256(size_t(B) * q.D * 4);
    l.total = l.hid + l.res + l.op + l.xz + l.xc + l.xdbl + l.so + l.scan + l.pa + l.pe + l.feat;
    return l;
}

// C [M, N] = a [M, K] . w^T (+ bias): planes operands, or fp32 operands split in the K loop where that kernel takes the shape,
// else the fp32 MFMA
int linear(int prec, bool planes, const void* a, const float* wf, const void* wp, const float* bias, float* C, long long M, int N, int K,
           unsigned* flag, hipStream_t st) {
    if (planes) return pope_launch_gemm_planes(pope_linear_params(LINEAR_PLANES, a, wp, bias, C, nullptr, int(M), N, K, EPI_BIAS, nullptr, nullptr, 0, flag), st);
    GemmParams g = pope_linear_params(LINEAR_F32, a, wf, bias, C, nullptr, int(M), N, K, EPI_BIAS, nullptr, nullptr, 0, flag);
    if (prec == POPE_PREC_F16X3 && pope_gemm_f16x3_supported(g)) return pope_launch_gemm_nt_f16x3(g, st);
    g.range_flag = nullptr;
    return pope_launch_gemm_nt_f32(g, st);
}

}  // namespace

int pope_vim_scan_chunk_len() { return SCAN_T; }

size_t pope_vim_scan_workspace(int B, int L, int E) {
    if (B <= 0 || L <= 0 || E <= 0) return 0;
    const size_t nch = (size_t(L) + SCAN_T - 1) / SCAN_T;
    return pope_align256(2 * size_t(B) * nch * E * NS * 4) + pope_align256(2 * size_t(B) * nch * E * 4);
}

int pope_vim_scan_check(const float* xc, const float* z, int ldz, const float* xdbl, const pope_vim_dir_weights* dirs, int B, int L, int E,
                        int R, const float* out_f32, const void* out_planes, const void* ws, size_t ws_bytes) {
    if (!xc || !z || !xdbl || !dirs || B <= 0 || B > 65535 || L <= 0 || E <= 0 || (E & 15) || R <= 0 || (R & 3) || R + 2 * NS > XS_MAX)
        return POPE_ERR_ARG;
    if (ldz < E || (ldz & 3) || (!out_f32) == (!out_planes) || (out_planes && (E & 31)) || E / SCAN_CH > 65535) return POPE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(xc) | reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(xdbl)) & 15) return POPE_ERR_ARG;
    for (int i = 0; i < 2; ++i)
        if (!dirs[i].dt_w || !dirs[i].dt_b || !dirs[i].A_log || !dirs[i].D) return POPE_ERR_ARG;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) return POPE_ERR_ARG;
    return ws_bytes < pope_vim_scan_workspace(B, L, E) ? POPE_ERR_WORKSPACE : POPE_OK;
}

int pope_launch_vim_scan(const float* xc, const float* z, int ldz, const float* xdbl, const pope_vim_dir_weights* dirs, int B, int L, int E,
                         int R, float* out_f32, void* out_planes, void* ws, unsigned* flag, hipStream_t st) {
    const int nch = (L + SCAN_T - 1) / SCAN_T;
    const long long M = 1ll * B * L;
    pope_carver cv{static_cast<char*>(ws)};
    float* hloc = cv.take<float>(2 * size_t(B) * nch * E * NS * 4);
    float* dsum = cv.take<float>(2 * size_t(B) * nch * E * 4);
    const DirPair p = dir_pair(dirs);
    const dim3 grid(nch, E / SCAN_CH, B), block(512);
    if (nch > 1) {
        hipLaunchKernelGGL(scan_state_kernel, grid, block, 0, st, xc, xdbl, p, L, E, R, M, nch, hloc, dsum);
        POPE_TRY(pope_check_launch());
    }
    if (out_planes)
        hipLaunchKernelGGL((scan_out_kernel<true>), grid, block, 0, st, xc, z, ldz, xdbl, p, L, E, R, M, nch, hloc, dsum, out_planes, flag);
    else
        hipLaunchKernelGGL((scan_out_kernel<false>), grid, block, 0, st, xc, z, ldz, xdbl, p, L, E, R, M, nch, hloc, dsum,
                           static_cast<void*>(out_f32), flag);
    return pope_check_launch();
}

int pope_vim_conv1d_check(const float* x, int ldx, const pope_vim_dir_weights* dirs, int B, int L, int E, const float* xc) {
    if (!x || !dirs || !xc || B <= 0 || L <= 0 || E <= 0 || (E & 3) || ldx < E || (ldx & 3)) return POPE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(xc)) & 15) return POPE_ERR_ARG;
    for (int i = 0; i < 2; ++i)
        if (!dirs[i].conv_w || !dirs[i].conv_b) return POPE_ERR_ARG;
    return POPE_OK;
}

int pope_launch_vim_conv1d(const float* x, int ldx, const pope_vim_dir_weights* dirs, int B, int L, int E, float* xc, hipStream_t st) {
    const long long M = 1ll * B * L, quads = 2 * M * (E / 4);
    hipLaunchKernelGGL(conv1d_silu_kernel, dim3(pope_grid_for(quads)), dim3(256), 0, st, x, ldx, dir_pair(dirs), L, E, M, xc, quads);
    return pope_check_launch();
}

int pope_vim_add_rmsnorm_check(const float* hidden, const float* w, const float* y_f32, const void* y_planes, long long rows, int D, float eps,
                               long long rs, long long r0) {
    if (!hidden || !w || (!y_f32) == (!y_planes) || rows <= 0 || rows > 0x7fffffffll * 4 || D <= 0 || (D & 3) || D > 2048) return POPE_ERR_ARG;
    if ((y_planes && (D & 31)) || !(eps > 0.f) || rs < 1 || r0 < 0) return POPE_ERR_ARG;
    return POPE_OK;
}

int pope_launch_vim_add_rmsnorm(const float* hidden, const float* res_in, float* res_out, const float* w, float* y_f32, void* y_planes,
                                long long rows, int D, float eps, long long rs, long long r0, unsigned* flag, hipStream_t st) {
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    if (y_planes)
        hipLaunchKernelGGL((add_rmsnorm_kernel<true>), grid, block, 0, st, hidden, res_in, res_out, w, y_planes, rows, D, eps, rs, r0, flag);
    else
        hipLaunchKernelGGL((add_rmsnorm_kernel<false>), grid, block, 0, st, hidden, res_in, res_out, w, static_cast<void*>(y_f32), rows, D, eps,
                           rs, r0, flag);
    return pope_check_launch();
}

size_t pope_vim_workspace(const pope_vim_weights* w, int B) {
    Geo q;
    return geometry(w, B, q) ? layout(q, B).total : 0;
}

int pope_vim_check(const VimArgs& a) {
    if (a.precision != POPE_PREC_F32_MFMA && a.precision != POPE_PREC_F16X3) return POPE_ERR_ARG;
    Geo q;
    if (!geometry(a.w, a.B, q) || !a.image || (reinterpret_cast<uintptr_t>(a.image) & 15)) return POPE_ERR_ARG;
    const pope_vim_weights& w = *a.w;
    const bool x3 = a.precision == POPE_PREC_F16X3;
    if (!w.patch_w || !w.patch_b || !w.cls || !w.pos || !w.norm_f_w || (x3 && !w.patch_wp)) return POPE_ERR_ARG;
    for (int i = 0; i < w.depth; ++i) {
        const pope_vim_layer_weights& k = w.layers_host[i];
        if (!k.norm_w || !k.in_proj_w || !k.out_proj_w || (x3 && (!k.in_proj_wp || !k.out_proj_wp))) return POPE_ERR_ARG;
        for (int d = 0; d < 2; ++d) {
            const pope_vim_dir_weights& v = k.dir[d];
            if (!v.conv_w || !v.conv_b || !v.x_proj_w || !v.dt_w || !v.dt_b || !v.A_log || !v.D) return POPE_ERR_ARG;
        }
    }
    if (a.logits && (!w.head_w || !w.head_b || w.num_classes <= 0 || (w.num_classes & 3))) return POPE_ERR_ARG;
    if (!a.ws || (reinterpret_cast<uintptr_t>(a.ws) & 255)) return POPE_ERR_ARG;
    return a.ws_bytes < layout(q, a.B).total ? POPE_ERR_WORKSPACE : POPE_OK;
}

int pope_launch_vim(const VimArgs& a, hipStream_t st) {
    POPE_TRY(pope_vim_check(a));
    const pope_vim_weights& w = *a.w;
    Geo q;
    geometry(a.w, a.B, q);
    const Layout lay = layout(q, a.B);
    pope_carver cv{static_cast<char*>(a.ws)};
    float* hid = cv.take<float>(lay.hid);
    float* res = cv.take<float>(lay.res);
    void* op = cv.take<void>(lay.op);
    float* xz = cv.take<float>(lay.xz);
    float* xc = cv.take<float>(lay.xc);
    float* xdbl = cv.take<float>(lay.xdbl);
    void* so = cv.take<void>(lay.so);
    void* scan_ws = cv.take<void>(lay.scan);
    void* pa = cv.take<void>(lay.pa);
    float* pe = cv.take<float>(lay.pe);
    float* feat_ws = cv.take<float>(lay.feat);
    const int prec = a.precision, B = a.B, D = q.D, E = q.E;
    const bool x3 = prec == POPE_PREC_F16X3;
    unsigned* flag = x3 ? a.range_flag : nullptr;
    const long long M = q.M;
    auto tap = [&](int i, const float* src) {
        if (!a.taps || !a.taps[i]) return POPE_OK;
        return hipMemcpyAsync(a.taps[i], src, size_t(M) * D * 4, hipMemcpyDeviceToDevice, st) == hipSuccess ? POPE_OK : POPE_ERR_LAUNCH;
    };
    auto norm = [&](const float* h, const float* rin, float* rout, const float* nw, bool planes, void* y, long long rows, long long rs, long long r0) {
        return pope_launch_vim_add_rmsnorm(h, rin, rout, nw, planes ? nullptr : static_cast<float*>(y), planes ? y : nullptr, rows, D, w.eps, rs, r0,
                                           flag, st);
    };
    {   // patch embedding: gather -> GEMM (K = 768) -> class token and pos_embed
        const long long quads = q.P * 192;
        if (x3)
            hipLaunchKernelGGL((patch_gather_kernel<true>), dim3(pope_grid_for(quads)), dim3(256), 0, st, a.image, pa, w.img, q.g, w.stride, quads, flag);
        else
            hipLaunchKernelGGL((patch_gather_kernel<false>), dim3(pope_grid_for(quads)), dim3(256), 0, st, a.image, pa, w.img, q.g, w.stride, quads, flag);
        POPE_TRY(pope_check_launch());
        POPE_TRY(linear(prec, x3, pa, w.patch_w, w.patch_wp, w.patch_b, pe, q.P, D, 768, flag, st));
        const long long tq = M * (D / 4);
        hipLaunchKernelGGL(place_tokens_kernel, dim3(pope_grid_for(tq)), dim3(256), 0, st, pe, w.cls, w.pos, hid, q.L, D, q.mid, tq);
        POPE_TRY(pope_check_launch());
        POPE_TRY(tap(0, hid));
    }
    const int tap_layer[3] = {0, w.depth / 2 - 1, w.depth - 1};
    for (int i = 0; i < w.depth; ++i) {
        const pope_vim_layer_weights& k = w.layers_host[i];
        POPE_TRY(norm(hid, i ? res : nullptr, res, k.norm_w, x3, op, M, 1, 0));
        for (int j = 0; j < 2; ++j)
            if (i > 0 && tap_layer[j] == i - 1) POPE_TRY(tap(1 + j, res));
        POPE_TRY(linear(prec, x3, op, k.in_proj_w, k.in_proj_wp, nullptr, xz, M, 2 * E, D, flag, st));
        POPE_TRY(pope_launch_vim_conv1d(xz, 2 * E, k.dir, B, q.L, E, xc, st));
        for (int d = 0; d < 2; ++d)
            POPE_TRY(linear(prec, false, xc + d * M * E, k.dir[d].x_proj_w, nullptr, nullptr, xdbl + d * M * q.XS, M, q.XS, E, flag, st));
        POPE_TRY(pope_launch_vim_scan(xc, xz + E, 2 * E, xdbl, k.dir, B, q.L, E, q.R, x3 ? nullptr : static_cast<float*>(so), x3 ? so : nullptr,
                                      scan_ws, flag, st));
        POPE_TRY(linear(prec, x3, so, k.out_proj_w, k.out_proj_wp, nullptr, hid, M, D, E, flag, st));
    }
    float* feat = a.features ? a.features : feat_ws;
    bool added = false;
    for (int j = 0; j < 3; ++j)
        if (a.taps && a.taps[1 + j] && tap_layer[j] == w.depth - 1) {
            if (!added) POPE_TRY(norm(hid, res, res, w.norm_f_w, false, xz, M, 1, 0));   // the whole hidden + residual for the tap
            added = true;
            POPE_TRY(tap(1 + j, res));
        }
    if (a.features || a.logits)   // norm_f on the class-token rows only
        POPE_TRY(pope_launch_vim_add_rmsnorm(added ? res : hid, added ? nullptr : res, nullptr, w.norm_f_w, feat, nullptr, B, D, w.eps, q.L, q.mid,
                                             nullptr, st));
    if (a.logits) POPE_TRY(linear(prec, false, feat, w.head_w, nullptr, w.head_b, a.logits, B, w.num_classes, D, flag, st));
    return POPE_OK;
}
