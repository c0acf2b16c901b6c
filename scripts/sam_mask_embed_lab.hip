// Lab: how the last layer of the SAM mask embedding (pope_amd/csrc/sam_prompt.hip) should fetch its 256 x 16 weights and how
// many channels a block should own.  Includes the shipped source, so the hidden values are the shipped code; only the channel
// loop is restated here, as lab_kernel<CH, LDS>: CH channels per block (the hidden values are recomputed 256 / CH times per
// pixel), weights through scalar loads (LDS = false, what ships) or copied to LDS once per block and read as broadcasts.
// Every variant's output is compared with the shipped kernel's bit for bit, then timed: device events around `reps`
// back-to-back launches, median over 15 windows.  One JSON line per (P, variant).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off scripts/sam_mask_embed_lab.hip -o scripts/sam_mask_embed_lab
#include "../pope_amd/csrc/sam_prompt.hip"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace {

template <int CH, bool LDS>
__global__ __launch_bounds__(THREADS) void lab_kernel(
    const float* __restrict__ masks, float* __restrict__ dense, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ g1, const float* __restrict__ s1, float eps1, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ g2, const float* __restrict__ s2, float eps2,
    const float* __restrict__ w3, const float* __restrict__ b3) {
    __shared__ __attribute__((aligned(16))) float ws[LDS ? CH * C2 : 4];
    __shared__ float bs[LDS ? CH : 4];
    const int p = blockIdx.x / TILES, tile = blockIdx.x % TILES;
    const int c0 = blockIdx.y * CH;
    if (LDS) {
        for (int i = threadIdx.x; i < CH * C2; i += THREADS) ws[i] = w3[c0 * C2 + i];
        for (int i = threadIdx.x; i < CH; i += THREADS) bs[i] = b3[c0 + i];
    }
    const int pix = tile * BLOCK_PIX + threadIdx.x * LANE_PIX;
    const int y = pix / GRID, x = pix % GRID;
    f32x4 h2[C2];
    mask_hidden(masks + size_t(p) * (SIDE * SIDE) + size_t(4 * y) * SIDE + 4 * x, w1, b1, g1, s1, eps1, w2, b2, g2, s2, eps2, h2);
    if (LDS) __syncthreads();
    float* out = dense + (size_t(p) * C3 + c0) * NPIX + pix;
#pragma unroll 4
    for (int c = 0; c < CH; ++c) {
        const float* wc = LDS ? ws + c * C2 : w3 + (c0 + c) * C2;
        f32x4 acc = splat(LDS ? bs[c] : b3[c0 + c]);
#pragma unroll
        for (int k = 0; k < C2; ++k) acc = fma4(wc[k], h2[k], acc);
        *reinterpret_cast<f32x4*>(out + size_t(c) * NPIX) = acc;
    }
}

#define HIP_OK(call) do { if ((call) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)

struct Dev {
    float *masks, *dense, *ref, *w[10];
};

template <int CH, bool LDS>
void launch_lab(const Dev& d, int P) {
    hipLaunchKernelGGL((lab_kernel<CH, LDS>), dim3(TILES * P, C3 / CH), dim3(THREADS), 0, nullptr, d.masks, d.dense, d.w[0], d.w[1], d.w[2],
                       d.w[3], 1e-6f, d.w[4], d.w[5], d.w[6], d.w[7], 1e-6f, d.w[8], d.w[9]);
}

void launch_shipped(const Dev& d, int P, float* out) {
    pope_sam_mask_embed_weights w{};
    w.mask_in_chans = C2; w.embed_dim = C3; w.grid = GRID; w.ln1_eps = w.ln2_eps = 1e-6f;
    w.conv1_w = d.w[0]; w.conv1_b = d.w[1]; w.ln1_w = d.w[2]; w.ln1_b = d.w[3];
    w.conv2_w = d.w[4]; w.conv2_b = d.w[5]; w.ln2_w = d.w[6]; w.ln2_b = d.w[7];
    w.conv3_w = d.w[8]; w.conv3_b = d.w[9];
    pope_launch_sam_mask_embed(&w, d.masks, P, out, nullptr);
}

template <typename F>
int timed(const char* name, int P, F launch, const Dev& d, const std::vector<float>& want, std::vector<float>& got) {
    const size_t n = size_t(P) * C3 * NPIX;
    HIP_OK(hipMemset(d.dense, 0xff, n * sizeof(float)));
    launch();
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(got.data(), d.dense, n * sizeof(float), hipMemcpyDeviceToHost));
    const bool same = std::memcmp(got.data(), want.data(), n * sizeof(float)) == 0;
    hipEvent_t a, b;
    HIP_OK(hipEventCreate(&a));
    HIP_OK(hipEventCreate(&b));
    const int reps = std::max(8, 512 / P);
    std::vector<float> us;
    for (int it = 0; it < 15; ++it) {
        HIP_OK(hipEventRecord(a, nullptr));
        for (int r = 0; r < reps; ++r) launch();
        HIP_OK(hipEventRecord(b, nullptr));
        HIP_OK(hipEventSynchronize(b));
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, a, b));
        us.push_back(ms * 1e3f / reps);
    }
    HIP_OK(hipGetLastError());
    std::sort(us.begin(), us.end());
    std::printf("{\"P\": %d, \"variant\": \"%s\", \"bit_equal_to_shipped\": %s, \"us_median\": %.2f, \"us_min\": %.2f, \"TBps\": %.3f}\n", P, name,
                same ? "true" : "false", us[us.size() / 2], us[0], double(P) * (SIDE * SIDE + C3 * NPIX) * 4 / (us[us.size() / 2] * 1e-6) / 1e12);
    std::fflush(stdout);
    HIP_OK(hipEventDestroy(a));
    HIP_OK(hipEventDestroy(b));
    return same ? 0 : 2;
}

}  // namespace

int main() {
    constexpr int PMAX = 64;
    const int sizes[10] = {16, 4, 4, 4, 256, 16, 16, 16, C3 * C2, C3};
    std::mt19937 rng(7);
    std::normal_distribution<float> nd(0.f, 1.f);
    Dev d{};
    for (int i = 0; i < 10; ++i) {
        std::vector<float> h(sizes[i]);
        const bool ln_w = i == 2 || i == 6;
        for (float& v : h) v = ln_w ? 1.f + 0.1f * nd(rng) : 0.25f * nd(rng);
        HIP_OK(hipMalloc(&d.w[i], h.size() * sizeof(float)));
        HIP_OK(hipMemcpy(d.w[i], h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    std::vector<float> hm(size_t(PMAX) * SIDE * SIDE);
    for (float& v : hm) v = -8.f + 6.f * nd(rng);
    const size_t nmax = size_t(PMAX) * C3 * NPIX;
    HIP_OK(hipMalloc(&d.masks, hm.size() * sizeof(float)));
    HIP_OK(hipMalloc(&d.dense, nmax * sizeof(float)));
    HIP_OK(hipMalloc(&d.ref, nmax * sizeof(float)));
    HIP_OK(hipMemcpy(d.masks, hm.data(), hm.size() * sizeof(float), hipMemcpyHostToDevice));
    std::vector<float> want(nmax), got(nmax);
    int rc = 0;
    for (int P : {1, 16, 64}) {
        launch_shipped(d, P, d.ref);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(want.data(), d.ref, size_t(P) * C3 * NPIX * sizeof(float), hipMemcpyDeviceToHost));
        rc |= timed("shipped (scalar loads, 64 ch)", P, [&] { launch_shipped(d, P, d.dense); }, d, want, got);
        rc |= timed("scalar loads, 32 ch", P, [&] { launch_lab<32, false>(d, P); }, d, want, got);
        rc |= timed("scalar loads, 128 ch", P, [&] { launch_lab<128, false>(d, P); }, d, want, got);
        rc |= timed("scalar loads, 256 ch", P, [&] { launch_lab<256, false>(d, P); }, d, want, got);
        rc |= timed("LDS, 64 ch", P, [&] { launch_lab<64, true>(d, P); }, d, want, got);
        rc |= timed("LDS, 128 ch", P, [&] { launch_lab<128, true>(d, P); }, d, want, got);
        rc |= timed("LDS, 256 ch", P, [&] { launch_lab<256, true>(d, P); }, d, want, got);
        if (rc & 1) return 1;   // a HIP error: nothing more is launched
    }
    return rc;
}
