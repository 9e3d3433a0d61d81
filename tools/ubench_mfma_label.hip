// What one label-overlap MFMA costs on this chip, and whether the FP4 form can stand in for two i8 ones (DESIGN 3.1 "The floor", row (d)):
//   * clocks per instruction of v_mfma_i32_16x16x64_i8 and of v_mfma_f32_16x16x128_f8f6f4 with E2M1 (FP4) operands for A and B
//     (cbsz:4 blgp:4, the unscaled form: both scales are 1), as one dependent chain (D of one is C of the next: the label chain of
//     k_scan_hist_r2) and as four independent chains (the issue interval), with one and with two waves per SIMD;
//   * exactness of the FP4 form as pass 1 would use it: 0 / 1 label bits as nibbles 0x0 / 0x2 (E2M1 0.0 / 1.0), lane (row, slot) holding
//     the 32 classes 32 slot .. 32 slot + 31, the chain started at the DENORMAL bit pattern 0x00010000.  Prints whether a zero overlap
//     leaves those bits untouched (the C operand is not flushed) and whether min_u32(bits, 0x10001) is 0x10000 | (overlap > 0) for
//     every pair of a tile, and whether the f32 value is the exact count up to 128.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench_mfma_label.hip -o tools/ubench_mfma_label.bin && tools/ubench_mfma_label.bin
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)
typedef int v4i __attribute__((ext_vector_type(4)));

#define MFMA_I8(D, C) asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %3" : "=&v"(D) : "v"(ra), "v"(rb), "v"(C))
#define MFMA_F4(D, C) asm volatile("v_mfma_f32_16x16x128_f8f6f4 %0, %1, %2, %3 cbsz:4 blgp:4" : "=&v"(D) : "v"(ra), "v"(rb), "v"(C))

// KIND 0: i8, 1: FP4.  NCH chains of 16 / NCH dependent instructions per iteration (NCH = 1: one dependent chain)
template <int KIND, int NCH>
__global__ __launch_bounds__(512) void k_chain(const v4i* in, v4i* out, int iters, unsigned long long* tim) {
    const int tid = threadIdx.x + blockIdx.x * blockDim.x;
    const v4i ra = in[(2 * tid) & 0xffff], rb = in[(2 * tid + 1) & 0xffff];
    v4i acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[c] = v4i{0, 0, 0, 0};
    const unsigned long long t0 = __builtin_readcyclecounter(), w0 = wall_clock64();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 16 / NCH; ++u)
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                v4i d;
                if (KIND == 0) MFMA_I8(d, acc[c]);
                else MFMA_F4(d, acc[c]);
                acc[c] = d;
            }
    }
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
    const unsigned long long t1 = __builtin_readcyclecounter(), w1 = wall_clock64();
    v4i s = acc[0];
#pragma unroll
    for (int c = 1; c < NCH; ++c) s += acc[c];
    out[tid] = s;
    if (threadIdx.x == 0 && blockIdx.x == 0) { tim[0] = t1 - t0; tim[1] = w1 - w0; }
}

// one tile: 16 items (A rows) x 16 queries (B columns), labels of 128 classes as four words each
__global__ __launch_bounds__(64) void k_exact(const uint32_t* ilab, const uint32_t* qlab, uint32_t* bits) {
    const int lane = threadIdx.x, row = lane & 15, slot = lane >> 4;
    const uint32_t wi = ilab[row * 4 + slot], wq = qlab[row * 4 + slot];
    v4i ra, rb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                    // nibble n of register j: class 32 slot + 4 n + j
        ra[j] = (int)(((wi >> j) & 0x11111111u) << 1);
        rb[j] = (int)(((wq >> j) & 0x11111111u) << 1);
    }
    v4i c = {0x10000, 0x10000, 0x10000, 0x10000}, d;
    asm volatile("s_nop 3\n\tv_mfma_f32_16x16x128_f8f6f4 %0, %1, %2, %3 cbsz:4 blgp:4\n\ts_nop 7\n\ts_nop 7" : "=&v"(d) : "v"(ra), "v"(rb), "v"(c));
#pragma unroll
    for (int j = 0; j < 4; ++j) bits[(4 * slot + j) * 16 + row] = (uint32_t)d[j];      // D[item 4 slot + j][query lane & 15]
}

int main() {
    v4i *din, *dout;
    unsigned long long* tim;
    std::vector<uint32_t> h(65536 * 4);
    uint32_t seed = 12345;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 4; };
    CK(hipMalloc(&din, h.size() * 4)); CK(hipMalloc(&dout, (size_t)256 * 512 * 16)); CK(hipMalloc(&tim, 16));
    for (int fill = 0; fill < 2; ++fill) {
        // operands: all zero, and random 0 / 1 label bits in the layout of each format (bytes 0 / 1 for i8, nibbles 0 / 2 for FP4)
        for (int kind = 0; kind < 2; ++kind) {
            for (auto& v : h) v = fill == 0 ? 0u : (kind == 0 ? rnd() & 0x01010101u : rnd() & 0x22222222u);
            CK(hipMemcpy(din, h.data(), h.size() * 4, hipMemcpyHostToDevice));
            for (int nch = 1; nch <= 4; nch += 3)
                for (int nthr = 256; nthr <= 512; nthr += 256) {
                    const int iters = 20000;
                    auto launch = [&]() {
                        if (kind == 0 && nch == 1) hipLaunchKernelGGL((k_chain<0, 1>), dim3(256), dim3(nthr), 0, 0, din, dout, iters, tim);
                        else if (kind == 0) hipLaunchKernelGGL((k_chain<0, 4>), dim3(256), dim3(nthr), 0, 0, din, dout, iters, tim);
                        else if (nch == 1) hipLaunchKernelGGL((k_chain<1, 1>), dim3(256), dim3(nthr), 0, 0, din, dout, iters, tim);
                        else hipLaunchKernelGGL((k_chain<1, 4>), dim3(256), dim3(nthr), 0, 0, din, dout, iters, tim);
                    };
                    launch();
                    CK(hipDeviceSynchronize());
                    launch();
                    CK(hipDeviceSynchronize());
                    unsigned long long ht[2];
                    CK(hipMemcpy(ht, tim, 16, hipMemcpyDeviceToHost));
                    printf("%-32s %-12s %s  %d waves/SIMD  clock %4.0f MHz  %6.2f clocks per instruction and SIMD\n",
                           kind == 0 ? "v_mfma_i32_16x16x64_i8" : "v_mfma_f32_16x16x128_f8f6f4 fp4", fill == 0 ? "zero" : "0/1 labels",
                           nch == 1 ? "dependent chain " : "4 indep. chains ", nthr / 256, ht[0] / (ht[1] / 100.0), (double)ht[0] / ((double)iters * 16 * (nthr / 256)));
                }
        }
    }
    // exactness: rows with no common class, one common class at chosen indices, all 128 common, random
    uint32_t il[16][4], ql[16][4], *dil, *dql, *dbits, bits[256];
    memset(il, 0, sizeof il); memset(ql, 0, sizeof ql);
    const int marks[8] = {0, 31, 32, 63, 64, 95, 96, 127};
    for (int r = 0; r < 8; ++r) il[r][marks[r] >> 5] = 1u << (marks[r] & 31);            // items 0-7: one class each
    for (int w = 0; w < 4; ++w) il[8][w] = 0xffffffffu;                                  // item 8: all classes; item 9: none
    for (int r = 10; r < 16; ++r) for (int w = 0; w < 4; ++w) il[r][w] = rnd() & rnd();
    for (int q = 0; q < 8; ++q) ql[q][marks[q] >> 5] = 1u << (marks[q] & 31);
    for (int w = 0; w < 4; ++w) ql[8][w] = 0xffffffffu;
    for (int q = 10; q < 16; ++q) for (int w = 0; w < 4; ++w) ql[q][w] = rnd() & rnd();
    CK(hipMalloc(&dil, sizeof il)); CK(hipMalloc(&dql, sizeof ql)); CK(hipMalloc(&dbits, sizeof bits));
    CK(hipMemcpy(dil, il, sizeof il, hipMemcpyHostToDevice)); CK(hipMemcpy(dql, ql, sizeof ql, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_exact, dim3(1), dim3(64), 0, 0, dil, dql, dbits);
    CK(hipMemcpy(bits, dbits, sizeof bits, hipMemcpyDeviceToHost));
    int bad_zero = 0, bad_min = 0, bad_count = 0, nzero = 0;
    for (int i = 0; i < 16; ++i)
        for (int q = 0; q < 16; ++q) {
            int cnt = 0;
            for (int w = 0; w < 4; ++w) cnt += __builtin_popcount(il[i][w] & ql[q][w]);
            const uint32_t b = bits[i * 16 + q];
            float f;
            memcpy(&f, &b, 4);
            if (cnt == 0) { ++nzero; bad_zero += b != 0x10000u; }
            else bad_count += f != (float)cnt;
            bad_min += (b < 0x10001u ? b : 0x10001u) != (0x10000u | (cnt > 0));
        }
    printf("FP4 label tile, chain started at the denormal 0x00010000: %d pairs without overlap, %d of them changed; %d wrong counts; %d wrong min(bits, 0x10001)\n",
           nzero, bad_zero, bad_count, bad_min);
    printf("sample bits: none %08x  one %08x  all-128 %08x\n", bits[9 * 16 + 9], bits[3 * 16 + 3], bits[8 * 16 + 8]);
    return bad_min != 0;
}
