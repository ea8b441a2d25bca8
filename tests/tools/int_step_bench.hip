// int_step_bench.hip -- the interior step of the wide walk loops in the instruction currency.  (development aid, not part of the product)
//
//   hipcc --offload-arch=gfx950 -O3 -Ibevyray_amd/csrc -o ab/int_step_bench tests/tools/int_step_bench.hip && ab/int_step_bench
//
// Sibling of pair_step_bench.hip.  The step is NOT copied here: the slab test and the decision are the piece the two wide loops share (brt_device.h,
// BRT_WIDE_INT_STEP) behind walk_wave_lds_asm's loads, so the step is timed exactly as the product runs it.  Every lane walks a chain of pair
// records in LDS (child L always pushed, child R never) that ends in a leaf after up to 256 steps; the host starts the chain over until the
// requested number of steps is reached.  Four settings on ONE CU:
//     alone, 1 wave per SIMD   (4 waves)            alone, 4 waves per SIMD   (16 waves)
//     1 + 1 filler per SIMD    (8 waves)            2 + 2 fillers per SIMD    (16 waves)
// A filler wave loops over the mix of the round's OTHER code by the counters of profiles/pmc_summary.json less the interior steps' own
// share: of 64 instructions 48 vector (3 fma to 1 select), 12 scalar, 1 LDS read and the wait, compare and branch of its loop; it runs until the
// last stepping wave has finished.  Time is the constant 100 MHz clock read by the stepping waves themselves (the longest of them), per
// step; "cycles" are that time at the nominal 2.4 GHz.  Instructions per step are counted from the step's own text.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brt_device.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)

constexpr int NREC = 256;              // 256 x 112 B = 28 KB at LDS address 0
constexpr unsigned REC = 112;
constexpr unsigned STACKS = NREC * REC;            // 16 waves x 4 KB of stack columns
constexpr unsigned DONE_WORD = STACKS + 16 * 4096; // how many stepping waves have finished
constexpr unsigned LDS_BYTES = DONE_WORD + 64;
static_assert(REC == brt::PAIR_BYTES, "the chain below is laid out for 112-byte pair records");

// one execution of the interior loop as walk_wave_lds_asm runs it: from the test at the loop's entry to the fall-through at its end
#define STEP_TEXT                                                                                                                      \
        "1:\n"                                                                                                                         \
        "ds_read_i16 %[pop], %[spa]\n"                                                                                                 \
        "v_mul_lo_u32 %[t0], %[cur], %[rec_bytes]\n"                                                                                   \
        "v_add_u32_e32 %[tx], %[t0], %[gofs_x]\n"                                                                                      \
        "ds_read_b128 v[100:103], %[tx]\n"                                                                                             \
        "v_add_u32_e32 %[ty], %[t0], %[gofs_y]\n"                                                                                      \
        "ds_read_b128 v[104:107], %[ty]\n"                                                                                             \
        "v_add_u32_e32 %[tz], %[t0], %[gofs_z]\n"                                                                                      \
        "ds_read_b128 v[108:111], %[tz]\n"                                                                                             \
        "ds_read_b64 v[112:113], %[t0] offset:96\n"                                                                                    \
        BRT_WIDE_INT_STEP("s_waitcnt lgkmcnt(3)\n", "s_waitcnt lgkmcnt(2)\n", "s_waitcnt lgkmcnt(1)\n", "s_waitcnt lgkmcnt(0)\n")

struct Mix { int vector, lds, scalar, all; };
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
    }
    return m;
}

__global__ void __launch_bounds__(1024) k_step(unsigned rounds, unsigned fillers, unsigned* out, unsigned long long* ticks) {
    extern __shared__ float lds[];
    for (int r = threadIdx.x; r < NREC; r += blockDim.x) {
        float* rec = lds + r * 28;
        for (int k = 0; k < 3; k++) {
            float* g = rec + 8 * k;           // G0 = { min L, min R, max L, max R }, G1 = { max L, max R, min L, min R }
            g[0] = -1e3f; g[1] = 1e6f; g[2] = 1e3f; g[3] = 2e6f;
            g[4] = 1e3f; g[5] = 2e6f; g[6] = -1e3f; g[7] = 1e6f;
        }
        reinterpret_cast<unsigned*>(rec)[24] = r + 1 < NREC ? (unsigned)(r + 1) : 0xfffffffeu;   // desc L: the next record, at the end a leaf
        reinterpret_cast<unsigned*>(rec)[25] = (unsigned)((r * 13 + 5) % NREC);                  // desc R (never taken)
    }
    if (threadIdx.x == 0) reinterpret_cast<unsigned*>(lds)[DONE_WORD / 4] = 0u;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const bool filler = fillers && ((wave >> 2) & 1u);            // waves 4-7 and 12-15: one resp. two on every SIMD
    const unsigned steppers = fillers ? nwaves / 2 : nwaves;
    if (filler) {
        float a = 1.0f + lane, b = 0.999f, c = 1e-3f, d = 2.0f, e = 3.0f, f;
        unsigned s = 0, s2;
        asm volatile(
            "v_cmp_lt_f32_e32 vcc, %[a], %[d]\n"
            "1:\n"
#define F4 "v_fma_f32 %[a], %[a], %[b], %[c]\n v_fma_f32 %[d], %[d], %[b], %[c]\n v_fma_f32 %[e], %[e], %[b], %[c]\n v_cndmask_b32_e32 %[e], %[e], %[a], vcc\n s_add_u32 %[s], %[s], 1\n"
            F4 F4 F4 F4 F4 F4 F4 F4 F4 F4 F4 F4
#undef F4
            "ds_read_b32 %[f], %[done]\n"
            "s_waitcnt lgkmcnt(0)\n"
            "v_readfirstlane_b32 %[s2], %[f]\n"
            "s_cmp_lt_u32 %[s2], %[need]\n"
            "s_cbranch_scc1 1b\n"
            : [a] "+v"(a), [d] "+v"(d), [e] "+v"(e), [f] "=&v"(f), [s] "+s"(s), [s2] "=&s"(s2)
            : [b] "v"(b), [c] "v"(c), [done] "v"(DONE_WORD), [need] "s"(steppers)
            : "vcc", "scc", "memory");
        if (out) out[blockIdx.x * blockDim.x + threadIdx.x] = __float_as_uint(a + d + e) + s;
        return;
    }
    const unsigned spa0 = STACKS + wave * 4096u + lane * 2u + 256u;
    unsigned acc = 0;
    const unsigned long long t_start = wall_clock64();
    for (unsigned round = 0; round < rounds; round++) {
        unsigned cur = (lane * 5u) & 63u, spa = spa0, t0, tx, ty, tz, pop, cnt;
        float closest = 1e5f, below;
        const float ox = 0.0f, oy = 0.0f, oz = 0.0f, ix = 1.0f, iy = 1.0f, iz = 1.0f;
        const unsigned gofs_x = 0u, gofs_y = 32u, gofs_z = 64u, rec_bytes = REC, thr = 0u;
        unsigned long long s_all, s_take, s_p2, s_any, s_both;
        asm volatile(
            "s_waitcnt lgkmcnt(0)\n"
            "s_mov_b64 %[s_all], exec\n"
            "v_add_u32_e32 %[below], -1, %[closest]\n"
            "v_cmpx_lt_i32_e32 vcc, -1, %[cur]\n"          // the loop's entry: EXEC = the lanes at an interior node
            STEP_TEXT
            "s_waitcnt lgkmcnt(0)\n"
            "s_mov_b64 exec, %[s_all]\n"
            : [cur] "+v"(cur), [spa] "+v"(spa), [below] "=&v"(below), [t0] "=&v"(t0), [tx] "=&v"(tx), [ty] "=&v"(ty), [tz] "=&v"(tz),
              [pop] "=&v"(pop), [cnt] "=&s"(cnt), [s_all] "=&s"(s_all), [s_take] "=&s"(s_take), [s_p2] "=&s"(s_p2), [s_any] "=&s"(s_any),
              [s_both] "=&s"(s_both)
            : [closest] "v"(closest), [gofs_x] "v"(gofs_x), [gofs_y] "v"(gofs_y), [gofs_z] "v"(gofs_z), [ox] "v"(ox), [oy] "v"(oy), [oz] "v"(oz),
              [ix] "v"(ix), [iy] "v"(iy), [iz] "v"(iz), [rec_bytes] "s"(rec_bytes), [thr] "s"(thr)
            : "vcc", "scc", "memory", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112",
              "v113");
        acc += cur + spa;                     // every lane ends at the leaf, 0xfffffffe, with its stack pointer where it was
    }
    const unsigned long long t_end = wall_clock64();
    if (lane == 0) {
        ticks[wave] = t_end - t_start;
        atomicAdd(reinterpret_cast<unsigned*>(lds) + DONE_WORD / 4, 1u);
    }
    if (out) out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

int main() {
    unsigned* d_out = nullptr;
    unsigned long long* d_ticks = nullptr;
    CHECK(hipMalloc(&d_out, 1024 * 4));
    CHECK(hipMalloc(&d_ticks, 16 * 8));
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_step), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
    constexpr Mix mix = count_step();
    const unsigned rounds = 4000;              // x 256 steps of the longest lane's chain
    std::printf("%d instructions per interior step (%d vector, %d LDS, %d scalar)\n", mix.all, mix.vector, mix.lds, mix.scalar);
    struct Case { const char* name; int threads; unsigned fillers; };
    const Case cases[] = {
        {"alone, 1 wave per SIMD", 256, 0u},
        {"alone, 4 waves per SIMD", 1024, 0u},
        {"1 wave + 1 filler per SIMD", 512, 1u},
        {"2 waves + 2 fillers per SIMD", 1024, 1u},
    };
    for (const Case& c : cases) {
        double best = 1e30;
        unsigned want = 0;
        for (int rep = 0; rep < 3; rep++) {
            CHECK(hipMemset(d_ticks, 0, 16 * 8));
            hipLaunchKernelGGL(k_step, dim3(1), dim3(c.threads), LDS_BYTES, 0, rounds, c.fillers, d_out, d_ticks);
            CHECK(hipDeviceSynchronize());
            unsigned long long t[16];
            unsigned o[64];
            CHECK(hipMemcpy(t, d_ticks, sizeof t, hipMemcpyDeviceToHost));
            CHECK(hipMemcpy(o, d_out, sizeof o, hipMemcpyDeviceToHost));
            unsigned long long longest = 0;
            for (unsigned long long x : t) longest = x > longest ? x : longest;
            const double ns = longest * 10.0 / ((double)rounds * NREC);
            if (rep && ns < best) best = ns;
            // lane 0 of wave 0: (leaf descriptor + untouched stack pointer) x rounds
            want = (0xfffffffeu + (STACKS + 256u)) * rounds;
            if (o[0] != want) { std::fprintf(stderr, "%s: the walk ended at %08x, not %08x\n", c.name, o[0], want); return 1; }
        }
        std::printf("  %-30s %7.1f ns per step  %6.0f cycles per step  %5.2f cycles per instruction\n", c.name, best, best * 2.4,
                    best * 2.4 / mix.all);
    }
    return 0;
}
