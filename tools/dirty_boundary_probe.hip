// Profiling-only: what does a kernel that ends with B freshly written bytes cost the dependent
// launch behind it, per store flavour?  ("the launch's end".)
//
// Kernel A has the step's launch shape: 2,048 one-wave workgroups, each writing one contiguous slab of
// B / 2,048 bytes through a per-wave buffer resource, 16 B per lane per instruction (1 KiB per wave-
// instruction), or 4 B per lane for the `wt4` flavour.  A trivial kernel that reads one word A wrote
// follows on the same stream.  200 such pairs are timed between two events.  Every slab comes out of
// one 203 MB working set (the FULL step's footprint at 65,536 fields), and the written window moves
// through it from pair to pair, so the Infinity Cache holds what it holds in the step and no pair
// rewrites lines the previous one left in the L2.
//
// Flavours (the `aux` argument of __builtin_amdgcn_raw_buffer_store_b128 on gfx950):
//   plain 0, nt 2, wt 16 (sc1, write-through), wtnt 18, wt4 = 16 with 4-B-per-lane stores.
// Output: one JSON object, microseconds per pair for every flavour and size, plus the `a_only` time
// of the same 200 launches of A without the trailing kernel and the empty pair (B = 0).
//
//   hipcc -O3 --offload-arch=gfx950 -o tools/_build/dirty_boundary_probe tools/dirty_boundary_probe.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "gfx950 only: the aux values are the gfx940+ cache-policy encoding"
#endif

constexpr int kWaves = 2048;
constexpr int kReps = 200;
constexpr size_t kWorkingSet = 203u * 1000u * 1000u;

typedef float f4v __attribute__((ext_vector_type(4)));

enum Flavour { kPlain = 0, kNt = 1, kWt = 2, kWtNt = 3, kWt4 = 4, kFlavours = 5 };
static const char* kNames[kFlavours] = {"plain", "nt", "wt", "wtnt", "wt4"};

// `per` bytes per wave (a multiple of 1 KiB), slab b at base + b * per.  The resource covers exactly
// the slab: a store past it would be dropped by the range check, and the host checks the whole window.
template <int AUX, bool NARROW>
__global__ __launch_bounds__(64) void write_kernel(char* base, uint32_t per, float value) {
  char* slab = base + (size_t)blockIdx.x * per;
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(slab, 0, (int)per, 0x00020000);
  const uint32_t lane = threadIdx.x;
  if constexpr (NARROW) {
    for (uint32_t off = 4u * lane; off < per; off += 256u)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(value), rsrc, (int)off, 0, AUX);
  } else {
    const f4v v = {value, value, value, value};
    for (uint32_t off = 16u * lane; off < per; off += 1024u)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned int, v),
                                             rsrc, (int)off, 0, AUX);
  }
}

// The dependent launch: 256 workgroups, each reads one word of what A wrote.
__global__ __launch_bounds__(64) void after_kernel(const float* written, float* out) {
  if (threadIdx.x == 0) out[blockIdx.x] = written[0] + 1.0f;
}

static void launch_a(int flavour, char* base, uint32_t per, float value, hipStream_t s) {
  const dim3 g(kWaves), b(64);
  switch (flavour) {
    case kPlain: hipLaunchKernelGGL((write_kernel<0, false>), g, b, 0, s, base, per, value); break;
    case kNt: hipLaunchKernelGGL((write_kernel<2, false>), g, b, 0, s, base, per, value); break;
    case kWt: hipLaunchKernelGGL((write_kernel<16, false>), g, b, 0, s, base, per, value); break;
    case kWtNt: hipLaunchKernelGGL((write_kernel<18, false>), g, b, 0, s, base, per, value); break;
    default: hipLaunchKernelGGL((write_kernel<16, true>), g, b, 0, s, base, per, value); break;
  }
}

#define CHECK(x)                                                             \
  do {                                                                       \
    hipError_t e_ = (x);                                                     \
    if (e_ != hipSuccess) {                                                  \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                \
      return 1;                                                              \
    }                                                                        \
  } while (0)

// Median over `rounds` timings of kReps (pairs or single launches), microseconds per repetition.
static int time_us(int flavour, char* ws, size_t bytes, bool with_after, float* out, hipStream_t s, double* us) {
  const uint32_t per = (uint32_t)(bytes / kWaves / 1024u * 1024u);
  const size_t window = (size_t)per * kWaves;
  if (window > kWorkingSet) return 1;
  const size_t room = kWorkingSet - window;  // the window's start moves within [0, room], 1-KiB aligned
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::vector<double> t;
  for (int round = 0; round < 5; ++round) {
    size_t start = 0;
    CHECK(hipEventRecord(e0, s));
    for (int r = 0; r < kReps; ++r) {
      launch_a(flavour, ws + start, per, (float)r, s);
      if (with_after) hipLaunchKernelGGL(after_kernel, dim3(256), dim3(64), 0, s, (const float*)(ws + start), out);
      start += window;
      if (start > room) start = room ? (start % room) / 1024u * 1024u : 0;
    }
    CHECK(hipEventRecord(e1, s));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipGetLastError());
    float ms = 0.0f;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (round) t.push_back(1000.0 * ms / kReps);  // the first round warms up
  }
  std::sort(t.begin(), t.end());
  *us = t[t.size() / 2];
  CHECK(hipEventDestroy(e0));
  CHECK(hipEventDestroy(e1));
  return 0;
}

int main() {
  char* ws;
  float* out;
  CHECK(hipMalloc(&ws, kWorkingSet));
  CHECK(hipMalloc(&out, 256 * sizeof(float)));
  CHECK(hipMemset(ws, 0, kWorkingSet));
  hipStream_t s;
  CHECK(hipStreamCreate(&s));
  const size_t sizes_mb[] = {0, 4, 16, 64, 187};
  printf("{\"waves\": %d, \"reps\": %d, \"working_set_bytes\": %zu, \"unit\": \"us per repetition, median of 4 rounds\"",
         kWaves, kReps, kWorkingSet);
  for (int with_after = 1; with_after >= 0; --with_after) {
    printf(",\n \"%s\": {", with_after ? "pair" : "a_only");
    for (int f = 0; f < kFlavours; ++f) {
      printf("%s\n  \"%s\": {", f ? "," : "", kNames[f]);
      bool first = true;
      for (size_t mb : sizes_mb) {
        double us = 0.0;
        if (time_us(f, ws, mb * 1000u * 1000u, with_after != 0, out, s, &us)) return 1;
        printf("%s\"%zu\": %.2f", first ? "" : ", ", mb, us);
        first = false;
      }
      printf("}");
    }
    printf("}");
  }
  printf("\n}\n");
  CHECK(hipDeviceSynchronize());
  return 0;
}
