// What the three flash-attention translation units (attention_f32.hip, attention_f16x3.hip, attention_f16.hip) share: the
// tile and LDS layout, the block decode, the lane maps, the last-tile key mask and the launchers' argument check.  Every kernel works in the same orientation: S^T = K . Q^T (lane (r, h) = (lane & 31, lane >> 5) holds 16 keys of
// query r per 32-key sub-tile), O^T += V^T . P^T with the score registers as the B operand.
#pragma once
#include "common.h"

namespace pope_attn {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int HD = 64;    // head dim (all DINOv2 archs)
constexpr int KT = 64;    // keys per LDS tile
// LDS row strides, chosen against bank conflicts (64 banks x 4 B):
constexpr int KST = 72;   // f16 K row (halves): 144 B = 9 x 16 B (odd) -> the ds_read_b128 of 32 consecutive rows is conflict-free
constexpr int VST = 96;   // f16 V row (halves): 192 B -> the 4 rows of a ds_read_b64_tr_b16 block hit disjoint banks
constexpr int OST = 68;   // fp32 row (floats): 17 x 16 B (odd) -> conflict-free ds_read_b128 / ds_write_b128; the epilogue staging row

__device__ __forceinline__ f32x16 mfma_f16(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f16x8 cat(f16x4 a, f16x4 b) { return f16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }
// One v_max3_f32 as inline asm: hipcc would otherwise canonicalise MFMA outputs before fmaxf (one extra v_max per element).
// The caller covers the XDL-write -> VALU-read wait states (the hazard recognizer does not look into inline asm).
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float d;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// the compiler-scheduled form, for kernels that must not hide reads of MFMA results inside asm
__device__ __forceinline__ float max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }

// Block decode.  1-D grid of n_qb query blocks per (image, head), XCD-aware: the query blocks of one (image, head) get
// consecutive logical ids, i.e. run on ONE XCD, so its private L2 serves their K/V re-reads (spread round-robin over the 8
// XCDs the fabric saw 4.6x the algorithmic bytes).
struct Block { int b, head, q0; };
__device__ __forceinline__ Block decode_block(int N, int heads, int qb) {
    const int n_qb = (N + qb - 1) / qb;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = logical / n_qb, head = bh % heads, b = bh / heads, q0 = (logical - bh * n_qb) * qb;
    return Block{b, head, q0};
}

// ds_read_b64_tr_b16 lane addressing for the V^T fragments (A operand of O^T += V^T . P^T), in halves from the start of a V
// stage with rows of VST halves: within a 16-lane group, lane 4q + p supplies row q, columns 4p..4p+3 of a 4-key x 16-d block
// and lane i receives column i (its d) of the 4 keys.  Block of lane l: keys 4 * (l >> 5) + q (+ 16 s + 8 + 32 u), d columns
// 16 * ((l >> 4) & 1) + 4 p (+ 32 dt).
__device__ __forceinline__ int tr_off(int lane, int h) { return (4 * h + ((lane & 15) >> 2)) * VST + 16 * ((lane >> 4) & 1) + 4 * (lane & 3); }

// the padded keys (>= N) of the last tile kt leave the softmax: d0 = scores of keys 0..31 of the tile, d1 = of keys 32..63
__device__ __forceinline__ void mask_tail(int kt, int h, int N, f32x16& d0, f32x16& d1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int key = kt * KT + mfma32_row(i, h);
        if (key >= N) d0[i] = -INFINITY;
        if (key + 32 >= N) d1[i] = -INFINITY;
    }
}

// The launchers' argument check; on success *grid = the 1-D grid size.  qb = queries per workgroup.  The kernels address one
// image's qkv rows (3 * heads * HD elements of qkv_elem_bytes each) through a buffer descriptor with a 32-bit extent: N rows,
// plus the tail_rows a kernel may address past the last one, must stay `margin` bytes below 4 GiB, or the extent would wrap.
static inline bool args_ok(int B, int N, int heads, int qb, int qkv_elem_bytes, int tail_rows, unsigned margin, const void* qkv,
                           const void* out, unsigned* grid) {
    if (!qkv || !out || B <= 0 || N <= 0 || heads <= 0) return false;
    if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return false;
    if ((size_t(N) + tail_rows) * 3 * heads * HD * qkv_elem_bytes >= (size_t(1) << 32) - margin) return false;
    const size_t blocks = size_t(B) * heads * ((N + qb - 1) / qb);
    if (blocks > 0x7fffffffull) return false;
    *grid = unsigned(blocks);
    return true;
}

}  // namespace pope_attn
