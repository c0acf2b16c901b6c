// Shared device/host helpers for the gfx950 (CDNA4, MI355X) kernels of the POPE hot path.
// Wave = 64 lanes everywhere; MFMA = v_mfma_f32_32x32x2_f32 (f32 in / f32 accumulate, exact
// k-ordered fmaf chain — the reference path is fp32 end to end).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define POPE_OK 0
#define POPE_ERR_ARG (-1)
#define POPE_ERR_LAUNCH (-2)
#define POPE_ERR_WORKSPACE (-3)

// C/D fragment map of every 32x32 MFMA on gfx950: register i of lane l holds
// row (i&3) + 8*(i>>2) + 4*(l>>5), column l&31.
__device__ __forceinline__ int mfma32_row(int i, int half) { return (i & 3) + 8 * (i >> 2) + 4 * half; }

__device__ __forceinline__ f32x16 mfma_32x32x2(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// Cross-lane exchange over lane distance 16 / 32 in ONE instruction (gfx950 v_permlane16/32_swap_b32): both results
// together hold, in every lane l, the values of lanes l and l ^ 16 (l ^ 32) — in a fixed order per lane, so a
// commutative combine (max, a + b) is deterministic.  (__shfl_xor is a ds_bpermute: address arithmetic + LDS trip.)
__device__ __forceinline__ void pope_xor16_pair(float v, float& a, float& b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
    // (elements are copied to scalars first: __builtin_bit_cast applied to r[1] directly reads element 0 with this clang)
    const unsigned r0 = r[0], r1 = r[1];
    a = __builtin_bit_cast(float, r0);
    b = __builtin_bit_cast(float, r1);
}
__device__ __forceinline__ void pope_xor32_pair(float v, float& a, float& b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
    // (elements are copied to scalars first: __builtin_bit_cast applied to r[1] directly reads element 0 with this clang)
    const unsigned r0 = r[0], r1 = r[1];
    a = __builtin_bit_cast(float, r0);
    b = __builtin_bit_cast(float, r1);
}

// Wave-uniform select that can never become control flow: the compiler turns chains of scalar ?: into branches at will,
// and a branch inside a software-pipelined K-step splits its basic block (the instruction-mix pins then no longer
// reach across it).  c != 0 ? a : b, all three in SGPRs.
__device__ __forceinline__ int pope_uniform_select(int c, int a, int b) {
    int r;   // readfirstlane: the operands are wave-uniform by contract; this pins them to SGPRs for the "s" constraints
    asm("s_cmp_lg_u32 %1, 0\n\ts_cselect_b32 %0, %2, %3"
        : "=s"(r)
        : "s"(__builtin_amdgcn_readfirstlane(c)), "s"(__builtin_amdgcn_readfirstlane(a)), "s"(__builtin_amdgcn_readfirstlane(b))
        : "scc");
    return r;
}

// Blocks b and b+8 share an XCD (round-robin dispatch).  Remap so that each XCD walks a
// contiguous chunk of the logical tile space (neighbouring tiles share operand panels in
// that XCD's private L2).  Bijective for any grid size; affects speed only.
__device__ __forceinline__ int xcd_remap(int bid, int nblocks) {
    const int q = nblocks >> 3, r = nblocks & 7, xcd = bid & 7;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}

// Per-device host state.  The reference keeps the matcher on cuda:1 and DINOv2 on cuda:0 in one process
// (pope_model_api.py:181-184), so everything the launchers cache is keyed by the CURRENT device (the Python
// binding makes the operand's device current around every call).
constexpr int POPE_MAX_DEVICES = 64;
static inline int pope_current_device() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= POPE_MAX_DEVICES) d = 0;
    return d;
}

// Number of CUs of the current device (cached per device; 256 on MI355X).  Host-side query, no sync.
static inline int pope_cu_count() {
    static std::atomic<int> cus[POPE_MAX_DEVICES];
    const int dev = pope_current_device();
    int n = cus[dev].load(std::memory_order_relaxed);
    if (!n) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

// One-time (per kernel AND device) opt-in for more than 64 KB of dynamic LDS.  `done` is a per-kernel bit mask of
// the devices that already have the attribute.
typedef std::atomic<unsigned long long> pope_dev_mask;
template <typename K>
static inline bool pope_opt_in_lds(K kernel, size_t bytes, pope_dev_mask& done) {
    const int dev = pope_current_device();
    if ((done.load(std::memory_order_acquire) >> dev) & 1ull) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes)) !=
        hipSuccess)
        return false;
    done.fetch_or(1ull << dev, std::memory_order_release);
    return true;
}

// ---- f16x3 operand split ------------------------------------------------------------------------------------------
// x = hi + lo with hi = f16(x) (RNE) and lo = f16(x - hi): x - hi is exact in fp32, so lo is its correctly rounded f16.
// v_fma_mixlo/mixhi_f16 read the f16 half of `hi` directly and write the f16 result into one half of the destination:
// four instructions produce the four lo halves of a quad (instead of 4 x v_cvt_f32_f16 + 4 x v_sub + 2 x v_cvt_pk) —
// bit-identical results, 6 instead of 12 VALU instructions per quad.
typedef _Float16 pope_f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 pope_f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 pope_f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ unsigned pope_split_lo_pair(float v0, float v1, unsigned hi_pair) {
    // two statements: the first result may share v0's register (v0 is dead after it) — the allocator decides; hi_pair
    // stays live across both, so the half-written destination never aliases it
    unsigned d;
    asm("v_fma_mixlo_f16 %0, -%1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(hi_pair), "v"(v0));
    asm("v_fma_mixhi_f16 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(d) : "v"(hi_pair), "v"(v1));
    return d;
}
__device__ __forceinline__ void pope_split4(f32x4 v, pope_f16x4& hi, pope_f16x4& lo) {
    typedef unsigned u32x2s __attribute__((ext_vector_type(2)));
    hi = __builtin_convertvector(v, pope_f16x4);  // 2 x v_cvt_pk_f16_f32 (RNE)
    const u32x2s hp = __builtin_bit_cast(u32x2s, hi);
    const u32x2s lp = {pope_split_lo_pair(v[0], v[1], hp[0]), pope_split_lo_pair(v[2], v[3], hp[1])};
    lo = __builtin_bit_cast(pope_f16x4, lp);
}

// ---- f16x3 planes layout (prose: kernels.h GemmParams::a_pl) ---------------------------------------------------------
// Column c of a planes row sits at half pope_planes_col(c) of the row's 2 * ld halves (hi plane), its lo twin 32 halves on.
constexpr __host__ __device__ int pope_planes_col(int c) { return (c >> 5) * 64 + (c & 31); }
// Split-and-store of 1, 2, 4 or 8 consecutive, ALREADY SCALED values at columns c.. of the planes row starting at `row`
// (c a multiple of the count: the values stay inside one 32-column chunk and the vector stores are aligned).
__device__ __forceinline__ void pope_planes_store(_Float16* row, int c, float y) {
    const _Float16 hi = _Float16(y);
    _Float16* o = row + pope_planes_col(c);
    o[0] = hi;
    o[32] = _Float16(y - float(hi));
}
__device__ __forceinline__ void pope_planes_store(_Float16* row, int c, f32x2 y) {
    const pope_f16x2 hi = __builtin_convertvector(y, pope_f16x2);
    _Float16* o = row + pope_planes_col(c);
    *reinterpret_cast<pope_f16x2*>(o) = hi;
    *reinterpret_cast<pope_f16x2*>(o + 32) = __builtin_convertvector(y - __builtin_convertvector(hi, f32x2), pope_f16x2);
}
__device__ __forceinline__ void pope_planes_store(_Float16* row, int c, f32x4 y) {
    pope_f16x4 hi, lo;
    pope_split4(y, hi, lo);
    _Float16* o = row + pope_planes_col(c);
    *reinterpret_cast<pope_f16x4*>(o) = hi;
    *reinterpret_cast<pope_f16x4*>(o + 32) = lo;
}
__device__ __forceinline__ void pope_planes_store(_Float16* row, int c, f32x4 y0, f32x4 y1) {
    pope_f16x4 h0, l0, h1, l1;
    pope_split4(y0, h0, l0);
    pope_split4(y1, h1, l1);
    _Float16* o = row + pope_planes_col(c);
    *reinterpret_cast<pope_f16x8*>(o) = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    *reinterpret_cast<pope_f16x8*>(o + 32) = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---- f16x3 range guard ------------------------------------------------------------------------------------------
// A planes producer converts value * scale to f16; a finite fp32 value whose scaled magnitude reaches 65520 rounds
// to +-inf there (and poisons everything downstream) although the fp32 reference is fine.  Every producer therefore
// tracks the largest scaled magnitude it converts and ORs its POPE_RANGE_* bit into a caller-provided device word;
// the host checks the word at its next synchronisation point and re-runs the work on the fp32 MFMA.
constexpr float POPE_F16_OVERFLOW = 65520.0f;  // smallest magnitude that RNE-rounds to f16 infinity
__device__ __forceinline__ void pope_range_flag(unsigned* flag, unsigned bit, bool bad) {
    if (flag && bad) (void)__hip_atomic_fetch_or(flag, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float pope_amax4(float m, f32x4 v) {
    return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1])),
                           __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v[2]), __builtin_fabsf(v[3])), m));
}
// two independent running maxima (m[0] over elements 0-1, m[1] over 2-3): no serial chain through one register
__device__ __forceinline__ void pope_amax4x2(f32x2& m, f32x4 v) {
    m[0] = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1])), m[0]);
    m[1] = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v[2]), __builtin_fabsf(v[3])), m[1]);
}
// fmax drops a NaN.  The plain-f16 GEMM epilogues keep, beside the maxima, a running sum of the values they convert: it is NaN
// from the first NaN on (or after inf - inf, which the maximum has caught; values below POPE_F16_OVERFLOW cannot sum to inf)
__device__ __forceinline__ void pope_nan_sum4(f32x2& s, f32x4 v) { s += f32x2{v[0], v[1]} + f32x2{v[2], v[3]}; }   // two packed adds
__device__ __forceinline__ bool pope_nan_seen(f32x2 s) { return !(s[0] + s[1] == s[0] + s[1]); }
__device__ __forceinline__ float pope_amax2(float m, f32x2 v) {
    return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1])), m);
}
// A converter's guard over the SCALED values it converts: bad() if and only if one of them was NaN or reached
// POPE_F16_OVERFLOW in magnitude.  fmax drops a NaN, so NaNs are caught apart: a sum of the values is NaN when one of
// them is (or when it is inf - inf, which the maximum has already caught).
struct pope_range_acc {
    float amax = 0.f;
    bool nan = false;
    __device__ __forceinline__ void add(float y) {
        amax = __builtin_fmaxf(amax, __builtin_fabsf(y));
        nan |= !(y == y);
    }
    __device__ __forceinline__ void add(f32x2 y) {
        amax = pope_amax2(amax, y);
        nan |= !(y[0] + y[1] == y[0] + y[1]);
    }
    __device__ __forceinline__ void add(f32x4 y) {
        amax = pope_amax4(amax, y);
        nan |= !((y[0] + y[1]) + (y[2] + y[3]) == (y[0] + y[1]) + (y[2] + y[3]));
    }
    __device__ __forceinline__ bool bad() const { return nan || !(amax < POPE_F16_OVERFLOW); }
};

static inline int pope_check_launch() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? POPE_OK : POPE_ERR_LAUNCH;
}
// return the first non-zero POPE_* code of a launch sequence
#define POPE_TRY(call) do { if (const int pope_rc_ = (call)) return pope_rc_; } while (0)

// Grid of a grid-stride kernel over `total` items: one block per `per_block` of them, at least one, at most 64 per CU.
static inline int pope_grid_for(long long total, int per_block = 256) {
    const long long b = (total + per_block - 1) / per_block, cap = 64ll * pope_cu_count();
    return int(b < 1 ? 1 : (b < cap ? b : cap));
}

// Workspaces are carved into 256-byte aligned pieces, by the size queries and the launchers alike.
static inline size_t pope_align256(size_t bytes) { return (bytes + 255) & ~size_t(255); }
struct pope_carver {
    char* at;
    template <typename T = void> T* take(size_t bytes) { char* r = at; at += pope_align256(bytes); return reinterpret_cast<T*>(r); }
};

// Launch of a kernel with more than 64 KB of dynamic LDS: the one-time opt-in (per kernel and device), the launch, its check.
template <auto KERNEL, typename... Args>
static inline int pope_launch_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args... args) {
    static pope_dev_mask lds_ok{0};
    if (!pope_opt_in_lds(KERNEL, lds_bytes, lds_ok)) return POPE_ERR_LAUNCH;
    hipLaunchKernelGGL(KERNEL, grid, block, lds_bytes, stream, args...);
    return pope_check_launch();
}

// ---- exact-erf GELU -------------------------------------------------------------------------------------------------
// nn.GELU() default = exact erf form, 0.5 x (1 + erf(x / sqrt 2)), evaluated branch-free (ocml erff: ~35 VALU
// per element with divergent range branches = ~20 % of an FC1 tile).  erfc via Abramowitz-Stegun 7.1.26 (|err| <= 1.5e-7):
// with z = |x|/sqrt2, t = 1/(1 + p z), q = 0.5 t P(t) exp(-z^2):
//   gelu(x) = x (1 - q) for x >= 0,  x q for x < 0   ==   relu(x) (1 - 2q) + x q.
// Max abs error vs the exact form over [-12, 12] in fp32: 4.7e-7 (one ulp at |x| ~ 4).  Every GEMM epilogue uses these two
// definitions, so the routes of one GEMM give the same bits.
namespace pope_gelu {
constexpr float P = 0.3275911f * 0.70710678118654752440f;
constexpr float A1 = 0.5f * 0.254829592f, A2 = 0.5f * -0.284496736f, A3 = 0.5f * 1.421413741f, A4 = 0.5f * -1.453152027f,
                A5 = 0.5f * 1.061405429f;
constexpr float NHL2E = -0.5f * 1.44269504088896340736f;  // exp(-x^2/2) = exp2(x * x * NHL2E)
}  // namespace pope_gelu

// on element PAIRS with packed f32 math (v_pk_fma_f32 / v_pk_mul_f32 for the polynomial)
__device__ __forceinline__ f32x2 pope_gelu_erf_pair(f32x2 x) {
    using namespace pope_gelu;
    f32x2 t, e, relu;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        t[i] = __builtin_amdgcn_rcpf(__builtin_fmaf(__builtin_fabsf(x[i]), P, 1.0f));
        relu[i] = __builtin_fmaxf(x[i], 0.0f);
    }
    const f32x2 arg = (x * NHL2E) * x;
    e[0] = __builtin_amdgcn_exp2f(arg[0]);
    e[1] = __builtin_amdgcn_exp2f(arg[1]);
    f32x2 poly = __builtin_elementwise_fma(t, f32x2{A5, A5}, f32x2{A4, A4});
    poly = __builtin_elementwise_fma(poly, t, f32x2{A3, A3});
    poly = __builtin_elementwise_fma(poly, t, f32x2{A2, A2});
    poly = __builtin_elementwise_fma(poly, t, f32x2{A1, A1});
    const f32x2 q = (poly * t) * e;
    return __builtin_elementwise_fma(relu, __builtin_elementwise_fma(q, f32x2{-2.f, -2.f}, f32x2{1.f, 1.f}), x * q);
}
// the same formula on one element
__device__ __forceinline__ float pope_gelu_erf(float x) {
    using namespace pope_gelu;
    const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(__builtin_fabsf(x), P, 1.0f));
    const float e = __builtin_amdgcn_exp2f((x * NHL2E) * x);
    float poly = __builtin_fmaf(t, A5, A4);
    poly = __builtin_fmaf(poly, t, A3);
    poly = __builtin_fmaf(poly, t, A2);
    poly = __builtin_fmaf(poly, t, A1);
    const float q = (poly * t) * e;
    return __builtin_fmaf(__builtin_fmaxf(x, 0.0f), __builtin_fmaf(q, -2.f, 1.f), x * q);
}

// ---- SwiGLU ---------------------------------------------------------------------------------------------------------
// dinov2/layers/swiglu_ffn.py:29-33: hidden = silu(gate) * value, silu(x) = x / (1 + exp(-x)), in fp32 with exp(-x) as
// exp2(-x log2 e) (the softmax kernels' stated deviation) and the quotient as x * rcp(.) (1 ulp, as the GELU's).  Finite for
// every finite gate: exp2 saturates to +inf (x * rcp(inf) = -0) or to 0 (x * rcp(1) = x), never inf / inf.  Every GEMM
// epilogue uses this one definition, so the routes of one GEMM give the same bits.  `inv` un-scales the f16x3 accumulators
// (1 on the fp32 MFMA), the biases are the gate's and the value's.
__device__ __forceinline__ f32x4 pope_swiglu4(f32x4 acc_gate, f32x4 acc_value, f32x4 bias_gate, f32x4 bias_value, float inv) {
    constexpr float NL2E = -1.44269504088896340736f;
    f32x4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float gt = __builtin_fmaf(acc_gate[e], inv, bias_gate[e]), vl = __builtin_fmaf(acc_value[e], inv, bias_value[e]);
        const float silu = gt * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(gt * NL2E));
        h[e] = silu * vl;
    }
    return h;
}
// The SwiGLU epilogues re-map the lanes over a wave's staged 32 x 64 block ([32 gate | 32 value] columns, kernels.h
// EPI_BIAS_SWIGLU): lane -> row (lane >> 3) + 8 i, hidden columns 4 (lane & 7) .. + 3, so that the eight lanes of a row write
// one whole 32-column chunk (64 B of hi + 64 B of lo halves, or 128 B of fp32).

