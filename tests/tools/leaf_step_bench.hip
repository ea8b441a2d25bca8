// leaf_step_bench.hip -- the leaf step of the wide walk loops in the instruction currency.  (development aid, not part of the product)
//
//   for n in 0 1 2 4 8 15; do
//     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Ibevyray_amd/csrc -DBRT_LEAF_ISSUE=$n -o ab/leaf_step_bench_$n tests/tools/leaf_step_bench.hip && ab/leaf_step_bench_$n
//   done
//
// Sibling of int_step_bench.hip.  Nothing is copied here: the kernel calls the product's walk_wave_lds_asm (brt_device.h) with every lane at a
// leaf, so the outer head, the leaf step and the way back are timed exactly as the product runs them, for the arm combination the file is
// built with (BRT_LEAF_ISSUE; bit 3 is the sampler's and changes nothing here).  Every lane's stack column holds 63 leaf descriptors above
// the DONE entry and its current node is a leaf: a call makes 64 leaf steps -- each entered from the outer head, the interior loop never
// runs -- and ends; the host repeats the call.  The 64 spheres lie behind one another in front of the ray, so a lane accepts the hits of
// its first steps and rejects the rest; every lane must end at sphere 0 with the t the host computes.  Two settings on ONE CU: 1 wave per
// SIMD (4 waves) and 4 waves per SIMD (16 waves).  Time is the constant 100 MHz clock read by the waves themselves (the longest of them),
// per step, the call's prologue and exit included (1/64 each); "cycles" are that time at the nominal 2.4 GHz.  Instructions per step are
// counted from the step's own text.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "brt_device.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)

constexpr unsigned NSPH = 64;                       // spheres { centre, r^2 } at LDS address 0
constexpr unsigned STACKS = NSPH * 16;              // 16 waves x 8 KB of stack columns: 64 entries of 128 bytes (64 lanes x 16 bits)
constexpr unsigned WAVE_STACK = 64 * 128;
constexpr unsigned LDS_BYTES = STACKS + 16 * WAVE_STACK;
constexpr unsigned STEPS = 64;                      // leaf steps of one call

// one leaf step as walk_wave_lds_asm runs it when it is entered from the outer head: from label 3 to the branch back to it
#if BRT_LEAF_ISSUE & 4
#define STEP_LANES BRT_WIDE_LEAF_LANES_HEAD
#else
#define STEP_LANES BRT_WIDE_LEAF_LANES_ALL
#endif
#define STEP_TEXT                                                                                                                      \
        BRT_WIDE_OUTER_HEAD                                                                                                            \
        STEP_LANES BRT_WIDE_LEAF_HEAD                                                                                                  \
        "v_lshl_add_u32 %[t0], v112, 4, %[sph]\n"                                                                                      \
        "ds_read_b128 v[100:103], %[t0]\n"                                                                                             \
        "ds_read_i16 %[cur], %[spa]\n"                                                                                                 \
        "s_waitcnt lgkmcnt(1)\n"                                                                                                       \
        BRT_WIDE_LEAF_TEST

struct Mix { int vector, lds, scalar, all; };
constexpr bool starts(const char* s, const char* p) {
    for (; *p; s++, p++) if (*s != *p) return false;
    return true;
}
// (up to the branch back to the outer head: the full forms behind it are out of line; of the head's two branches neither is taken)
constexpr Mix count_step() {
    constexpr char text[] = STEP_TEXT;
    Mix m{0, 0, 0, 0};
    int start = 0;
    for (int i = 0; text[i]; i++) {
        if (text[i] != '\n') continue;
        int b = start;
        while (text[b] == ' ') b++;
        start = i + 1;
        if (text[i - 1] == ':') continue;             // a label
        m.all++;
        if (text[b] == 'v') m.vector++; else if (text[b] == 'd') m.lds++; else m.scalar++;
        if (starts(text + b, "s_branch 3b")) break;
    }
    return m;
}

__host__ __device__ inline void sphere_of(unsigned i, float* s) {
    s[0] = 0.05f * (float)(i % 7u); s[1] = 0.03f * (float)(i % 5u); s[2] = 4.0f + 0.5f * (float)i; s[3] = 1.0f;
}

__global__ void __launch_bounds__(1024) k_leaf(unsigned rounds, unsigned* out, unsigned long long* ticks) {
    extern __shared__ float lds[];
    for (unsigned i = threadIdx.x; i < NSPH; i += blockDim.x) sphere_of(i, lds + 4 * i);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned short* column = reinterpret_cast<unsigned short*>(lds) + (STACKS + wave * WAVE_STACK) / 2 + lane;
    column[0] = 0xffffu;                                                              // DONE
    for (unsigned e = 1; e < STEPS; e++) column[64 * e] = (unsigned short)(0xc000u | ((lane + e) % NSPH));   // single-sphere leaves
    __syncthreads();
    const unsigned spa0 = STACKS + wave * WAVE_STACK + lane * 2u + (STEPS - 1u) * 128u;
    const brt::f3 o = brt::mk3(0.0f, 0.0f, 0.0f), d = brt::mk3(0.0f, 0.0f, 1.0f), inv = brt::mk3(1.0f, 1.0f, 1.0f);
    unsigned acc = 0, last_idx = 0;
    float last_t = 0.0f;
    const unsigned long long t_start = wall_clock64();
    for (unsigned round = 0; round < rounds; round++) {
        unsigned cur = 0xffffc000u | (lane % NSPH), spa = spa0, idx = 0xffffffffu;
        float closest = brt::kInf;
        brt::walk_wave_lds_asm(cur, spa, closest, idx, 0u, 32u, 64u, o, inv, d, 1.0f, 0u, 0u, brt::kLeafVote);
        acc += cur + spa;
        last_idx = idx;
        last_t = closest;
    }
    const unsigned long long t_end = wall_clock64();
    if (lane == 0) ticks[wave] = t_end - t_start;
    unsigned* o3 = out + 3 * (blockIdx.x * blockDim.x + threadIdx.x);
    o3[0] = acc; o3[1] = last_idx; o3[2] = __float_as_uint(last_t);
}

int main() {
    unsigned* d_out = nullptr;
    unsigned long long* d_ticks = nullptr;
    CHECK(hipMalloc(&d_out, 1024 * 3 * 4));
    CHECK(hipMalloc(&d_ticks, 16 * 8));
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_leaf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
    constexpr Mix mix = count_step();
    const unsigned rounds = 16000;             // x 64 steps
    // what every lane must end with: the nearest of the 64 spheres, by the shader's expressions (correctly rounded sqrt and divide)
    float want_t = 3.40282347e+38f;
    unsigned want_idx = 0xffffffffu;
    for (unsigned i = 0; i < NSPH; i++) {
        float s[4];
        sphere_of(i, s);
        const float h = (0.0f * s[0] + 0.0f * s[1]) + 1.0f * s[2];
        const float c = ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) - s[3];
        const float disc = h * h - 1.0f * c;
        const float t = (h - std::sqrt(disc)) / 1.0f;
        if (t > 0.001f && t < want_t) { want_t = t; want_idx = i; }
    }
    std::printf("BRT_LEAF_ISSUE=%d: %d instructions per leaf step with its outer head (%d vector, %d LDS, %d scalar)\n", (int)BRT_LEAF_ISSUE,
                mix.all, mix.vector, mix.lds, mix.scalar);
    struct Case { const char* name; int threads; };
    const Case cases[] = {{"1 wave per SIMD", 256}, {"4 waves per SIMD", 1024}};
    for (const Case& c : cases) {
        double best = 1e30;
        for (int rep = 0; rep < 3; rep++) {
            CHECK(hipMemset(d_ticks, 0, 16 * 8));
            hipLaunchKernelGGL(k_leaf, dim3(1), dim3(c.threads), LDS_BYTES, 0, rounds, d_out, d_ticks);
            CHECK(hipGetLastError());
            CHECK(hipDeviceSynchronize());
            unsigned long long t[16];
            static unsigned o[1024 * 3];
            CHECK(hipMemcpy(t, d_ticks, sizeof t, hipMemcpyDeviceToHost));
            CHECK(hipMemcpy(o, d_out, sizeof(unsigned) * 3 * c.threads, hipMemcpyDeviceToHost));
            unsigned long long longest = 0;
            for (unsigned long long x : t) longest = x > longest ? x : longest;
            const double ns = longest * 10.0 / ((double)rounds * STEPS);
            if (rep && ns < best) best = ns;
            for (int l = 0; l < c.threads; l++) {
                unsigned want_bits;
                std::memcpy(&want_bits, &want_t, 4);
                if (o[3 * l + 1] != want_idx || o[3 * l + 2] != want_bits) {
                    std::fprintf(stderr, "%s: thread %d ended at sphere %u with t bits %08x, not sphere %u with %08x\n", c.name, l, o[3 * l + 1],
                                 o[3 * l + 2], want_idx, want_bits);
                    return 1;
                }
            }
        }
        std::printf("  %-20s %7.1f ns per step  %6.0f cycles per step  %5.2f cycles per instruction\n", c.name, best, best * 2.4, best * 2.4 / mix.all);
    }
    return 0;
}
