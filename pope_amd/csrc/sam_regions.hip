// SAM automatic mask generator, small-region clean-up of a batch of bit-packed masks (segment_anything/utils/amg.py:
// remove_small_regions called twice per mask by automatic_mask_generator.py:postprocess_small_regions): holes below
// min_area filled, then islands below min_area removed, 8-connectivity, plus the box and the area of the cleaned mask.
//
// Connected components by union-find on WORD-RUNS: a word-run is a maximal run of set bits inside one 32-bit word of a row
// (at most 16 per word), found with ctz / clz on the word; its key is row * pitch16 + (x of its first bit >> 1) with
// pitch16 = 16 * words per row: two word-runs of a row never start at adjacent x, so the key is unique, it grows in raster
// order, and the label / counter arrays need H * pitch16 entries (half a word per pixel), of which only the entries of
// word-run starts are ever touched.  A word-run is joined with the word-run that ends at bit 31 of the word to its left (W)
// and with every word-run of the row above that has a bit in [first - 1, last + 1] (NW, N, NE), read from the word above
// and one bit of each of its neighbours.  The root of a set is its smallest key (atomicMin, retried from the value it
// returns), i.e. the word-run that holds the component's first pixel in raster order: the tie rule of the reference
// ("the first of the largest") needs nothing more.  Sizes are integer atomic adds of run lengths into the root's counter,
// so no result depends on the order in which threads arrive.
//
// One workgroup per mask runs every phase of both passes with a workgroup barrier in between, so a mask's labels stay on
// one CU and no protocol between workgroups exists.  Labels and counters are only ever accessed with agent-scope atomics
// (loads and stores included): they are served by the L2, never by a vector L1 line that predates an atomic update.
// The grid is min(n, kChunk) workgroups; workgroup b cleans masks b, b + grid, .. with slot b of the workspace.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kChunk = 32;            // masks in flight = workspace slots
constexpr long long kMaxPixels = 1ll << 24;

struct RegionPass {
    const unsigned* src;   // [H, Wp] words this pass labels (after ^ flip, & valid)
    unsigned* dst;         // [H, Wp] words this pass writes
    int* label;            // [H * pitch16]
    int* count;            // [H * pitch16]
    int H, Wp, pitch16, min_area;
    unsigned last_valid;   // valid bits of the last word of a row
    unsigned flip;         // ~0u: the complement is labelled (holes), 0: the mask itself (islands)
};

// what a workgroup reduces per mask
struct RegionShared {
    int small, big;                 // some component is below min_area / is not
    unsigned long long best;        // islands, all small: max of (size << 32 | ~key), i.e. the largest, then the first
    int area, xmin, ymin, xmax, ymax;
    int changed_holes;
};

struct DeviceOps {
    static __device__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ void store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ int fetch_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ void add(int* p, int v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    // the workgroup's reductions (LDS)
    static __device__ void wg_or(int* p, int v) { atomicOr(p, v); }
    static __device__ void wg_add(int* p, int v) { atomicAdd(p, v); }
    static __device__ void wg_min(int* p, int v) { atomicMin(p, v); }
    static __device__ void wg_max(int* p, int v) { atomicMax(p, v); }
    static __device__ void wg_max64(unsigned long long* p, unsigned long long v) { atomicMax(p, v); }
};

__host__ __device__ inline unsigned pass_word(const RegionPass& c, int y, int i) {
    if (y < 0 || i < 0 || i >= c.Wp) return 0u;
    return (c.src[size_t(y) * c.Wp + i] ^ c.flip) & (i == c.Wp - 1 ? c.last_valid : ~0u);
}

// length of the run of set bits of `w` that starts at bit a (bit a set, bit a - 1 clear or a == 0)
__host__ __device__ inline int run_length(unsigned w, int a) {
    const unsigned z = ~(w >> a);           // the shift brings zeros in at the top, so z != 0 unless a == 0 and w is full
    return z ? __builtin_ctz(z) : 32;
}
__host__ __device__ inline unsigned run_mask(int a, int len) { return len == 32 ? ~0u : ((1u << len) - 1u) << a; }
// first bit of the run of set bits of `w` that holds bit c
__host__ __device__ inline int run_start(unsigned w, int c) {
    const unsigned z = ~w & ((1u << c) - 1u);
    return z ? 32 - __builtin_clz(z) : 0;
}
__host__ __device__ inline int run_key(const RegionPass& c, int y, int i, int a) { return y * c.pitch16 + i * 16 + (a >> 1); }

template <class Ops>
__host__ __device__ inline int find_root(int* label, int x) {
    for (int p; (p = Ops::load(label + x)) != x;) x = p;
    return x;
}

// Labels only ever decrease and always point to a key of the same component, so a retry from the value atomicMin returns
// loses no link: if label[a] was no longer a, the former parent `old` is joined with b in the next round.
template <class Ops>
__host__ __device__ inline void unite(int* label, int a, int b) {
    for (;;) {
        a = find_root<Ops>(label, a);
        b = find_root<Ops>(label, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = Ops::fetch_min(label + a, b);
        if (old == a) return;
        a = old;
    }
}

// every word-run start is its own root with an empty counter
template <class Ops>
__host__ __device__ inline void phase_init(const RegionPass& c, int tid, int nt) {
    const int words = c.H * c.Wp;
    for (int w = tid; w < words; w += nt) {
        const int y = w / c.Wp, i = w - y * c.Wp;
        const unsigned b = pass_word(c, y, i);
        for (unsigned s = b & ~(b << 1); s; s &= s - 1) {
            const int k = run_key(c, y, i, __builtin_ctz(s));
            Ops::store(c.label + k, k);
            Ops::store(c.count + k, 0);
        }
    }
}

template <class Ops>
__host__ __device__ inline void phase_union(const RegionPass& c, int tid, int nt) {
    const int words = c.H * c.Wp;
    for (int w = tid; w < words; w += nt) {
        const int y = w / c.Wp, i = w - y * c.Wp;
        const unsigned b = pass_word(c, y, i);
        if (!b) continue;
        const unsigned left = pass_word(c, y, i - 1);
        const unsigned up[3] = {pass_word(c, y - 1, i - 1), pass_word(c, y - 1, i), pass_word(c, y - 1, i + 1)};
        // bit p of the window = pixel 32 i - 1 + p of the row above, p = 0 .. 33
        const unsigned long long window = (unsigned long long)(up[0] >> 31) | ((unsigned long long)up[1] << 1)
                                          | ((unsigned long long)(up[2] & 1u) << 33);
        for (unsigned s = b & ~(b << 1); s; s &= s - 1) {
            const int a = __builtin_ctz(s), len = run_length(b, a), me = run_key(c, y, i, a);
            if (a == 0 && (left >> 31)) unite<Ops>(c.label, me, run_key(c, y, i - 1, run_start(left, 31)));
            // pixels first - 1 .. last + 1 of the row above are window bits a .. a + len + 1
            unsigned long long t = window & (((1ull << (len + 2)) - 1ull) << a);
            while (t) {
                const int p = __builtin_ctzll(t);
                const int j = p == 0 ? 0 : (p == 33 ? 2 : 1), bit = (p + 31) & 31;     // which of up[], which bit of it
                unite<Ops>(c.label, me, run_key(c, y - 1, i - 1 + j, run_start(up[j], bit)));
                t &= t + (t & (0ull - t));     // drop the lowest run of window bits: its word-runs are joined by their own W links
            }
        }
    }
}

// Path compression and sizes.  A thread takes a contiguous span of words: neighbouring word-runs mostly share a root, so
// a span's lengths are summed in a register and leave as one add per change of root.
template <class Ops>
__host__ __device__ inline void phase_count(const RegionPass& c, int tid, int nt) {
    const int words = c.H * c.Wp, span = (words + nt - 1) / nt;
    const int w1 = (tid + 1) * span < words ? (tid + 1) * span : words;
    int cur = -1, acc = 0;
    for (int w = tid * span; w < w1; ++w) {
        const int y = w / c.Wp, i = w - y * c.Wp;
        const unsigned b = pass_word(c, y, i);
        for (unsigned s = b & ~(b << 1); s; s &= s - 1) {
            const int a = __builtin_ctz(s), k = run_key(c, y, i, a);
            const int root = find_root<Ops>(c.label, k);
            Ops::store(c.label + k, root);
            if (root != cur) {
                if (acc) Ops::add(c.count + cur, acc);
                cur = root;
                acc = 0;
            }
            acc += run_length(b, a);
        }
    }
    if (acc) Ops::add(c.count + cur, acc);
}

// islands: is there a component of min_area or more, and which small one is the largest (the first of them on a tie)
template <class Ops>
__host__ __device__ inline void phase_roots(const RegionPass& c, RegionShared* sh, int tid, int nt) {
    const int words = c.H * c.Wp;
    int small = 0, big = 0;
    unsigned long long best = 0ull;
    for (int w = tid; w < words; w += nt) {
        const int y = w / c.Wp, i = w - y * c.Wp;
        const unsigned b = pass_word(c, y, i);
        for (unsigned s = b & ~(b << 1); s; s &= s - 1) {
            const int k = run_key(c, y, i, __builtin_ctz(s));
            if (Ops::load(c.label + k) != k) continue;
            const int n = Ops::load(c.count + k);
            if (n < c.min_area) {
                small = 1;
                const unsigned long long v = ((unsigned long long)(unsigned)n << 32) | (0xffffffffu - (unsigned)k);
                best = v > best ? v : best;
            } else {
                big = 1;
            }
        }
    }
    if (small) { Ops::wg_or(&sh->small, 1); Ops::wg_max64(&sh->best, best); }
    if (big) Ops::wg_or(&sh->big, 1);
}

// holes: fill every small component of the complement
template <class Ops>
__host__ __device__ inline void phase_fill(const RegionPass& c, RegionShared* sh, int tid, int nt) {
    const int words = c.H * c.Wp;
    int small = 0;
    for (int w = tid; w < words; w += nt) {
        const int y = w / c.Wp, i = w - y * c.Wp;
        const unsigned b = pass_word(c, y, i);
        unsigned fill = 0u;
        for (unsigned s = b & ~(b << 1); s; s &= s - 1) {
            const int a = __builtin_ctz(s);
            const int root = Ops::load(c.label + run_key(c, y, i, a));
            if (Ops::load(c.count + root) < c.min_area) fill |= run_mask(a, run_length(b, a));
        }
        small |= fill != 0u;
        // b is the complement inside the valid bits: the mask itself is the rest of them
        c.dst[w] = ((i == c.Wp - 1 ? c.last_valid : ~0u) & ~b) | fill;
    }
    if (small) Ops::wg_or(&sh->small, 1);
}

// islands: drop the small components (all of them small: keep `best`), then the area and the box of what is left
template <class Ops>
__host__ __device__ inline void phase_keep(const RegionPass& c, RegionShared* sh, int keep_key, int tid, int nt) {
    const int words = c.H * c.Wp;
    int area = 0, xmin = 0x7fffffff, ymin = 0x7fffffff, xmax = -1, ymax = -1;
    for (int w = tid; w < words; w += nt) {
        const int y = w / c.Wp, i = w - y * c.Wp;
        const unsigned b = pass_word(c, y, i);
        unsigned out = 0u;
        for (unsigned s = b & ~(b << 1); s; s &= s - 1) {
            const int a = __builtin_ctz(s);
            const int root = Ops::load(c.label + run_key(c, y, i, a));
            if (root == keep_key || Ops::load(c.count + root) >= c.min_area) out |= run_mask(a, run_length(b, a));
        }
        c.dst[w] = out;
        if (out) {
            area += __builtin_popcount(out);
            const int x0 = i * 32 + __builtin_ctz(out), x1 = i * 32 + 31 - __builtin_clz(out);
            xmin = x0 < xmin ? x0 : xmin;
            xmax = x1 > xmax ? x1 : xmax;
            ymin = y < ymin ? y : ymin;
            ymax = y > ymax ? y : ymax;
        }
    }
    if (area) {
        Ops::wg_add(&sh->area, area);
        Ops::wg_min(&sh->xmin, xmin); Ops::wg_min(&sh->ymin, ymin);
        Ops::wg_max(&sh->xmax, xmax); Ops::wg_max(&sh->ymax, ymax);
    }
}

__host__ __device__ inline void shared_reset(RegionShared* sh) {
    sh->small = sh->big = 0;
    sh->best = 0ull;
    sh->area = 0;
    sh->xmin = sh->ymin = 0x7fffffff;
    sh->xmax = sh->ymax = -1;
    sh->changed_holes = 0;
}
// key of the island that stays although it is small: only when every island is small
__host__ __device__ inline int kept_small_key(const RegionShared* sh) {
    return (sh->small && !sh->big) ? int(0xffffffffu - unsigned(sh->best & 0xffffffffull)) : -1;
}
// unchanged, box (batched_mask_to_box: inclusive maxima, zeros for an empty mask) and area of one mask
__host__ __device__ inline void write_results(const RegionShared* sh, int* unchanged, int* box, int* area) {
    *unchanged = !(sh->changed_holes || sh->small);
    const bool empty = sh->area == 0;
    box[0] = empty ? 0 : sh->xmin; box[1] = empty ? 0 : sh->ymin;
    box[2] = empty ? 0 : sh->xmax; box[3] = empty ? 0 : sh->ymax;
    *area = sh->area;
}

struct RegionsK {
    const unsigned* packed;
    unsigned* packed_out;
    int *unchanged, *boxes, *area;
    int *label, *count;      // [slots][H * pitch16]
    int n, H, W, Wp, min_area;
};

__global__ __launch_bounds__(kThreads) void sam_small_regions_kernel(RegionsK k) {
    __shared__ RegionShared sh;
    const int tid = threadIdx.x;
    const size_t words = size_t(k.H) * k.Wp, keys = words * 16;
    RegionPass c;
    c.H = k.H; c.Wp = k.Wp; c.pitch16 = k.Wp * 16; c.min_area = k.min_area;
    c.last_valid = (k.W & 31) ? (1u << (k.W & 31)) - 1u : ~0u;
    c.label = k.label + blockIdx.x * keys;
    c.count = k.count + blockIdx.x * keys;
    for (int m = blockIdx.x; m < k.n; m += gridDim.x) {     // workgroup-uniform: every barrier below is met by all threads
        c.dst = k.packed_out + m * words;
        if (tid == 0) shared_reset(&sh);
        // holes: the complement of the input, filled into dst
        c.src = k.packed + m * words; c.flip = ~0u;
        phase_init<DeviceOps>(c, tid, kThreads);
        __syncthreads();
        phase_union<DeviceOps>(c, tid, kThreads);
        __syncthreads();
        phase_count<DeviceOps>(c, tid, kThreads);
        __syncthreads();
        phase_fill<DeviceOps>(c, &sh, tid, kThreads);
        __syncthreads();
        if (tid == 0) { sh.changed_holes = sh.small; sh.small = 0; }
        // islands: the filled mask, cleaned in place
        c.src = c.dst; c.flip = 0u;
        phase_init<DeviceOps>(c, tid, kThreads);
        __syncthreads();
        phase_union<DeviceOps>(c, tid, kThreads);
        __syncthreads();
        phase_count<DeviceOps>(c, tid, kThreads);
        __syncthreads();
        phase_roots<DeviceOps>(c, &sh, tid, kThreads);
        __syncthreads();
        phase_keep<DeviceOps>(c, &sh, kept_small_key(&sh), tid, kThreads);
        __syncthreads();
        if (tid == 0) write_results(&sh, k.unchanged + m, k.boxes + size_t(m) * 4, k.area + m);
        __syncthreads();     // sh is reset for the next mask only after its results have left
    }
}

inline bool geometry_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W < kMaxPixels; }
inline size_t slot_keys(int H, int W) { return size_t(H) * size_t((W + 31) / 32) * 16; }

}  // namespace

int pope_sam_small_regions_chunk() { return kChunk; }

size_t pope_sam_small_regions_workspace(int n, int H, int W) {
    if (n <= 0 || !geometry_ok(H, W)) return 0;
    const int slots = n < kChunk ? n : kChunk;
    return 2 * pope_align256(size_t(slots) * slot_keys(H, W) * sizeof(int));
}

int pope_sam_small_regions_check(const SamRegionsArgs& a) {
    if (a.n < 0 || a.min_area < 0 || !geometry_ok(a.H, a.W)) return POPE_ERR_ARG;
    if (a.n == 0) return POPE_OK;
    if (!a.packed || !a.packed_out || !a.unchanged || !a.boxes || !a.area || !a.ws) return POPE_ERR_ARG;
    // in place is fine (a mask is read and written by its own workgroup only); any other overlap is not
    const size_t bytes = size_t(a.n) * a.H * ((a.W + 31) / 32) * sizeof(unsigned);
    const char *in = reinterpret_cast<const char*>(a.packed), *out = reinterpret_cast<const char*>(a.packed_out);
    if (in != out && in < out + bytes && out < in + bytes) return POPE_ERR_ARG;
    if (a.ws_bytes < pope_sam_small_regions_workspace(a.n, a.H, a.W)) return POPE_ERR_WORKSPACE;
    return POPE_OK;
}

int pope_launch_sam_small_regions(const SamRegionsArgs& a, hipStream_t stream) {
    POPE_TRY(pope_sam_small_regions_check(a));
    if (a.n == 0) return POPE_OK;
    const int slots = a.n < kChunk ? a.n : kChunk;
    RegionsK k = {};
    k.packed = a.packed; k.packed_out = a.packed_out; k.unchanged = a.unchanged; k.boxes = a.boxes; k.area = a.area;
    k.n = a.n; k.H = a.H; k.W = a.W; k.Wp = (a.W + 31) / 32; k.min_area = a.min_area;
    pope_carver ws{static_cast<char*>(a.ws)};
    const size_t bytes = size_t(slots) * slot_keys(a.H, a.W) * sizeof(int);
    k.label = ws.take<int>(bytes);
    k.count = ws.take<int>(bytes);
    hipLaunchKernelGGL(sam_small_regions_kernel, dim3(slots), dim3(kThreads), 0, stream, k);
    return pope_check_launch();
}
