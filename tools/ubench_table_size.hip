// Micro-benchmark behind DESIGN "odd-multiple table rows": the inner loop of the bucket walk (g1_walk of kernels_g1.hip.h — a chain of
// XYZZ mixed additions, one random 128-byte table record gathered per addition) over tables of growing size: the bit-row table of the
// 6145-point SRS with 1, 2, 4, 8, 16 and 32 blocks of multiples is 201, 402, 804, 1608, 3216 and 6432 MB, against the 256 MB Infinity Cache.
// The records are 135190 distinct points repeated over the table (what is gathered does not matter to the memory system, only where).
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I dot_ring_amd/csrc tools/ubench_table_size.hip -o tools/ubench_table_size
//   run:   tools/ubench_table_size [K [lanes]]
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "kernels_g1.hip.h"

using namespace dr;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

// record i of the big table (128 bytes, 96 used) = small point i % n_small
__global__ __launch_bounds__(256) void k_fill_table(const uint32_t* __restrict__ small, uint32_t n_small, uint32_t* __restrict__ table, uint32_t records) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= records) return;
    const uint32_t* s = small + (size_t)(i % n_small) * 24;
    uint32_t* d = table + (size_t)i * 32;
    for (int j = 0; j < 24; j++) d[j] = s[j];
    for (int j = 24; j < 32; j++) d[j] = 0;
}

// entries as the sort leaves them: a random record below `records` | a random sign << 31, lane-major per chain step
__global__ __launch_bounds__(256) void k_fill_entries(uint32_t* __restrict__ idx, size_t count, uint32_t records, uint64_t seed) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint64_t x = (i + 1) * 0x9e3779b97f4a7c15ull + seed;                     // splitmix64
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27; x *= 0x94d049bb133111ebull; x ^= x >> 31;
    idx[i] = (uint32_t)((x >> 1) % records) | ((uint32_t)(x & 1) << 31);
}

__global__ __launch_bounds__(256) void k_walk(const uint32_t* __restrict__ table, const uint32_t* __restrict__ idx, uint32_t K, uint32_t lanes,
                                              uint32_t* __restrict__ out) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= lanes) return;
    store_xyzz(out, lane, g1_walk(table, 32u, idx, lane, K * lanes, 0u, lanes));     // entries lane, lane + lanes, ...: K of them
}

int main(int argc, char** argv) {
    const uint32_t K = argc > 1 ? (uint32_t)atoi(argv[1]) : 64u, lanes = argc > 2 ? (uint32_t)atoi(argv[2]) : 1u << 20;
    const uint32_t n_small = 6145 * 22;
    if (K == 0 || lanes == 0 || lanes % 256 || (uint64_t)K * lanes >= (1ull << 31)) { printf("K x lanes must be below 2^31, lanes a multiple of 256\n"); return 1; }
    static const uint32_t GEN[24] = {
        0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu, 0x9774b905u, 0xc3688c4fu, 0x4fa9ac0fu, 0x2695638cu, 0x3197d794u, 0x17f1d3a7u,
        0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu, 0xd5d00af6u, 0xfcf5e095u, 0x741d8ae4u, 0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u};
    uint32_t *d_seed, *d_small, *d_table, *d_idx, *d_out;
    CK(hipMalloc(&d_seed, sizeof GEN));
    CK(hipMemcpy(d_seed, GEN, sizeof GEN, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_g1_bases_to_mont, dim3(1), dim3(256), 0, 0, d_seed, 1u);
    CK(hipMalloc(&d_small, (size_t)n_small * 96));
    hipLaunchKernelGGL(k_g1_synth_bases, dim3((n_small + 255) / 256), dim3(256), 0, 0, d_small, n_small, 1u, d_seed);
    const uint32_t blocks[] = {1, 2, 4, 8, 16, 32};
    const uint32_t max_records = 6145u * 256u * 32u;             // 50.3 M records of 128 bytes: 6.4 GB (a record index stays below 2^31)
    const size_t count = (size_t)K * lanes;
    CK(hipMalloc(&d_table, (size_t)max_records * 128));
    CK(hipMalloc(&d_idx, count * 4));
    CK(hipMalloc(&d_out, (size_t)lanes * 192));
    hipLaunchKernelGGL(k_fill_table, dim3((max_records + 255) / 256), dim3(256), 0, 0, d_small, n_small, d_table, max_records);
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    printf("%u lanes x %u additions, one 128-byte record gathered per addition; kernel time by HIP events, median of 5\n", lanes, K);
    for (uint32_t m : blocks) {
        const uint32_t records = 6145u * 256u * m;
        std::vector<float> ms(5);
        for (int rep = 0; rep < 6; rep++) {             // (the first run warms up)
            hipLaunchKernelGGL(k_fill_entries, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, d_idx, count, records, (uint64_t)(rep * 8 + m));
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(k_walk, dim3(lanes / 256), dim3(256), 0, 0, d_table, d_idx, K, lanes, d_out);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float t = 0;
            CK(hipEventElapsedTime(&t, e0, e1));
            if (rep) ms[rep - 1] = t;
        }
        std::sort(ms.begin(), ms.end());
        printf("%u block%s of rows, %8u records, %7.1f MB: %7.2f ms = %5.2f G additions/s (min %.2f, max %.2f ms)\n", m, m > 1 ? "s" : " ", records,
               records * 128.0 / 1e6, ms[2], (double)count / ms[2] / 1e6, ms[0], ms[4]);
    }
    return 0;
}
