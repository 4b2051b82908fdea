// Microbenchmark (dev tool, not part of the library): LDS fill/read rates per CU on gfx950.
//   mode 0: global_load_lds_dwordx4 (LDS-DMA) from an L2-hot 64 KB window, 8 waves
//   mode 1: global_load_dwordx4 -> ds_write_b128 (register staging), 8 waves
//   mode 2: ds_read_b128 only, 8 waves
//   mode 3: waves 0-3 LDS-DMA, waves 4-7 ds_read_b128 concurrently
//   mode 4: waves 0-3 register staging, waves 4-7 ds_read_b128
// `lds_fill probe` runs none of them: it checks the immediate-offset rule of the LDS-DMA load (probe_imm below).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define GLDS16(g, l) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g), (__attribute__((address_space(3))) void*)(l), 16, 0, 0)

template <int MODE>
__global__ __launch_bounds__(512) void k(const char* src, float* out, int iters) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const char* g = src + (size_t)blockIdx.x * 65536 + lane * 16;
    f32x4 acc = {0, 0, 0, 0};
    const bool writer = MODE == 0 || MODE == 1 || ((MODE == 3 || MODE == 4) && wave < 4);
    const bool reader = MODE == 2 || ((MODE == 3 || MODE == 4) && wave >= 4);
    for (int it = 0; it < iters; ++it) {
        if (writer) {
            // each wave moves 8 KB per iteration: 8 pieces of 1 KB
            if constexpr (MODE == 0 || MODE == 3) {
#pragma unroll
                for (int i = 0; i < 8; ++i) GLDS16(g + ((wave * 8 + i) & 63) * 1024, lds + (wave * 8 + i) * 1024);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else {
                f32x4 v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const f32x4*>(g + ((wave * 8 + i) & 63) * 1024);
#pragma unroll
                for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(lds + (wave * 8 + i) * 1024 + lane * 16) = v[i];
            }
        }
        if (reader) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(lds + 65536 + ((wave * 8 + i) & 63) * 1024 + lane * 16);
                acc += v;
            }
        }
    }
    if (acc.x == 12345.f) out[threadIdx.x] = acc.x + acc.y + acc.z + acc.w;
}

template <int MODE> static void run(const char* name, const char* d_src, float* d_out, int iters, double bytes_w, double bytes_r) {
    hipFuncSetAttribute((const void*)k<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    k<MODE><<<256, 512, 131072>>>(d_src, d_out, 10);
    hipEventRecord(e0);
    k<MODE><<<256, 512, 131072>>>(d_src, d_out, iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("%-44s %8.3f ms  write %7.1f GB/s/CU  read %7.1f GB/s/CU\n", name, ms, bytes_w * iters / ms / 1e6, bytes_r * iters / ms / 1e6);
}
// `lds_fill probe`: what the immediate offset of global_load_lds_dwordx4 is added to.  One wave, two pieces behind ONE
// M0 write: piece 0 with offset:0, piece 1 with offset:1024 and a lane offset of 4096 - 1024.  If the immediate goes to
// BOTH the LDS destination and the global address, LDS[1024 + x] = src[4096 + x] (and LDS[x] = src[x]); src holds its own
// word index, LDS starts as 0xFFFFFFFF, so any other rule shows in the words printed.
__global__ __launch_bounds__(64) void probe_imm(const char* src, uint32_t* out) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const uint32_t lane = threadIdx.x;
    uint32_t* w = reinterpret_cast<uint32_t*>(lds);
    for (uint32_t i = lane; i < 2048; i += 64) w[i] = 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t lds_addr = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds);
    const uint32_t v0 = lane * 16u, v1 = lane * 16u + 4096u - 1024u;
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %3\n\t"
                 "global_load_lds_dwordx4 %2, %3 offset:1024\n\t"
                 "s_waitcnt vmcnt(0)"
                 :: "s"(lds_addr), "v"(v0), "v"(v1), "s"(src) : "memory");
    __syncthreads();
    for (uint32_t i = lane; i < 2048; i += 64) out[i] = w[i];
}
static int run_probe() {
    const uint32_t nsrc = 4096;   // words: 16 KB
    uint32_t h_src[nsrc], h_out[2048];
    for (uint32_t i = 0; i < nsrc; ++i) h_src[i] = i;
    char* d_src; uint32_t* d_out;
    hipMalloc(&d_src, sizeof h_src); hipMemcpy(d_src, h_src, sizeof h_src, hipMemcpyHostToDevice);
    hipMalloc(&d_out, sizeof h_out);
    probe_imm<<<1, 64, 8192>>>(d_src, d_out);
    if (hipMemcpy(h_out, d_out, sizeof h_out, hipMemcpyDeviceToHost) != hipSuccess) { printf("probe: the copy back failed\n"); return 1; }
    int bad = 0;
    for (uint32_t i = 0; i < 256; ++i) bad += h_out[i] != i;                  // piece 0: LDS[0, 1024) = src[0, 1024)
    for (uint32_t i = 0; i < 256; ++i) bad += h_out[256 + i] != 1024 + i;     // piece 1: LDS[1024, 2048) = src[4096, 5120)
    for (uint32_t i = 512; i < 2048; ++i) bad += h_out[i] != 0xFFFFFFFFu;     // nothing else written
    printf("probe: LDS words [0] %u [255] %u | [256] %u [511] %u | [512] %#x   (expected 0 255 | 1024 1279 | 0xffffffff)\n",
           h_out[0], h_out[255], h_out[256], h_out[511], h_out[512]);
    printf("probe: the immediate offset is added to the LDS destination AND the global address: %s\n", bad ? "NO" : "yes");
    return bad != 0;
}
int main(int argc, char** argv) {
    if (argc > 1 && argv[1][0] == 'p') return run_probe();
    char* d_src; float* d_out;
    hipMalloc(&d_src, 256 * 65536); hipMemset(d_src, 1, 256 * 65536); hipMalloc(&d_out, 4096);
    const int iters = 20000;
    run<0>("0: LDS-DMA fill, 8 waves", d_src, d_out, iters, 65536, 0);
    run<1>("1: global_load + ds_write_b128, 8 waves", d_src, d_out, iters, 65536, 0);
    run<2>("2: ds_read_b128, 8 waves", d_src, d_out, iters, 0, 65536);
    run<3>("3: 4 waves LDS-DMA + 4 waves ds_read_b128", d_src, d_out, iters, 32768, 32768);
    run<4>("4: 4 waves reg-staged + 4 waves ds_read_b128", d_src, d_out, iters, 32768, 32768);
    return 0;
}
