// mfma_f16_layout_probe.hip - operand lane layout and issue rate of v_mfma_f32_16x16x32_f16 on gfx950 (the split-f16 persistent
// forward, csrc/opnet_xcd_split_kernels.hip), checked with exact integer data on one wave.
// build: hipcc --offload-arch=gfx950 -O3 -o tools/probes/mfma_f16_layout_probe tools/probes/mfma_f16_layout_probe.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// the layout the kernel assumes: lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15], j = 0..7;
// D[row 4 (l >> 4) + r][col l & 15] in register r
__host__ __device__ inline int a_val(int i, int k) { return (i * 7 + k * 3) % 5 - 2; }
__host__ __device__ inline int b_val(int k, int n) { return (k * 5 + n * 11) % 7 - 3; }

__global__ void layout(float *out)
{
    const int l = threadIdx.x, r = l & 15, u = l >> 4;
    h8 a, b;
    for (int j = 0; j < 8; ++j) { a[j] = (_Float16)a_val(r, 8 * u + j); b[j] = (_Float16)b_val(8 * u + j, r); }
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    for (int q = 0; q < 4; ++q) out[l * 4 + q] = c[q];
}

// CHAINS accumulators, 12 MFMAs per iteration: cycles per MFMA of one wave (1 wave per SIMD with 256 threads, 2 with 512)
template <int CHAINS>
__global__ void rate(float *out, long long *cyc, int iters)
{
    const int l = threadIdx.x & 63;
    h8 a, b;
    for (int j = 0; j < 8; ++j) { a[j] = (_Float16)(0.001f * (l + j)); b[j] = (_Float16)(0.5f - 0.01f * j); }
    f32x4 c[4];
    for (int i = 0; i < 4; ++i) c[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const long long t0 = clock64();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int k = 0; k < 12; ++k) c[k % CHAINS] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c[k % CHAINS], 0, 0, 0);
    }
    const long long t1 = clock64();
    float s = 0.f;
    for (int i = 0; i < 4; ++i) s += c[i][0] + c[i][1] + c[i][2] + c[i][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0 && blockIdx.x == 0) *cyc = t1 - t0;
}

int main()
{
    float *d; long long *dc;
    if (hipMalloc(&d, 1 << 20) != hipSuccess || hipMalloc(&dc, 16) != hipSuccess) { printf("no device memory\n"); return 1; }
    float h[256];
    layout<<<1, 64>>>(d);
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { printf("layout kernel failed\n"); return 1; }
    int bad = 0;
    for (int l = 0; l < 64; ++l)
        for (int q = 0; q < 4; ++q) {
            const int i = 4 * (l >> 4) + q, n = l & 15;
            int want = 0;
            for (int k = 0; k < 32; ++k) want += a_val(i, k) * b_val(k, n);
            if (h[l * 4 + q] != (float)want) { if (bad < 8) printf("lane %d reg %d: got %g want %d\n", l, q, h[l * 4 + q], want); ++bad; }
        }
    printf("layout A[l&15][8(l>>4)+j], B[8(l>>4)+j][l&15], D[4(l>>4)+r][l&15]: %s\n", bad ? "NO" : "yes");
    const int iters = 2000;
    long long c;
#define RUN(CH, THR) do { rate<CH><<<1, THR>>>(d, dc, iters); (void)hipDeviceSynchronize(); (void)hipMemcpy(&c, dc, 8, hipMemcpyDeviceToHost); \
        printf("chains %d, %d waves/CU: %.2f clock64 cycles per MFMA per wave\n", CH, THR / 64, (double)c / (12.0 * iters)); } while (0)
    RUN(1, 64); RUN(2, 64); RUN(4, 64); RUN(2, 256); RUN(2, 512);
    return bad ? 1 : 0;
}
