// Residency probe: how many 256-lane workgroups with S bytes of dynamic LDS are resident per CU -- i.e. in what units the CU hands out
// LDS?  Every workgroup spins ~100 us on the constant-rate clock (bounded loop, waits for nobody); the grid has 6 workgroups per CU.
// Time / T = 2 -> 3 per CU, 3 -> 2 per CU, 6 -> 1 per CU.  hipcc -O2 --offload-arch=gfx950 tools/lds_residency.hip -o tools/lds_residency
// (profiles/block_pass_teams/lds_granule.txt is its output on an MI355X.)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
__global__ __launch_bounds__(256) void probe(unsigned long long ticks, unsigned* sink)
{
    extern __shared__ unsigned lds[];
    lds[threadIdx.x] = threadIdx.x;
    __syncthreads();
    const unsigned long long t0 = wall_clock64();
    unsigned acc = 0;
    for (int i = 0; i < 4000000; i++) {
        acc += lds[(threadIdx.x + i) & 255];
        if (wall_clock64() - t0 >= ticks) break;
    }
    if (acc == 0xFFFFFFFFu) *sink = acc;
}
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s -> %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
int main()
{
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    printf("CUs %d sharedMemPerBlock %zu maxSharedMemoryPerMultiProcessor %zu\n", p.multiProcessorCount, p.sharedMemPerBlock, p.maxSharedMemoryPerMultiProcessor);
    unsigned* sink;
    CK(hipMalloc(&sink, 4));
    hipError_t a = hipFuncSetAttribute((const void*)probe, hipFuncAttributeMaxDynamicSharedMemorySize, 163840);
    printf("set attribute: %s\n", hipGetErrorString(a));
    int rate = 0;
    CK(hipDeviceGetAttribute(&rate, hipDeviceAttributeWallClockRate, 0));  // kHz
    const unsigned long long ticks = (unsigned long long)rate / 10;        // 100 us
    printf("wall clock %d kHz, %llu ticks per workgroup\n", rate, ticks);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const unsigned sizes[] = {1024, 40960, 53760, 54272, 54613, 79744, 80640, 81920, 81921, 83200};
    for (unsigned s : sizes) {
        int occ = -1;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, probe, 256, s);
        for (int rep = 0; rep < 2; rep++) {
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(probe, dim3(p.multiProcessorCount * 6), dim3(256), s, 0, ticks, sink);
            CK(hipGetLastError());
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms = 0;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep) printf("dyn LDS %6u B: %.3f ms = %.2f T   (runtime occupancy query: %d per CU)\n", s, ms, ms / 0.1f, occ);
        }
    }
    return 0;
}
