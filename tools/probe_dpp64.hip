// Hardware probe for the pair kernel's fused half-wide broadcasts (gfx950):
//  (1) values: v_fmac_f64_dpp with a row_newbcast:N source against
//      fma(bcast, +-own, acc) with the broadcast taken by __shfl from lane
//      16 row + N, for every N and both signs, bitwise; and the whole path the
//      kernel uses -- rep16 (one v_permlane16_swap_b32 per dword) plus the fused
//      FMA -- for every source lane s < 32 of a half; and two fused FMAs back to
//      back on an accumulator and a factor written by the instructions right
//      before them (no wait state but the DPP source's).  Random doubles, signed
//      zeros, denormals, infinities and NaNs; all 64 lanes active, then each
//      32-lane half alone.
//  (2) cycles: 256 independent instructions between two s_memtime reads, at one
//      and at three waves per SIMD: plain v_fmac_f64, the fused form, the
//      replicate step of one double, and a uniform-address ds_read_b128 with
//      the two FMAs that consume it.
// One short run; build: hipcc -O3 --offload-arch=gfx950 tools/probe_dpp64.hip -o tools/probe_dpp64
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

__device__ inline void rep16(double v, double& lo, double& hi) {
  const unsigned vl = (unsigned)__double2loint(v), vh = (unsigned)__double2hiint(v);
  const auto l = __builtin_amdgcn_permlane16_swap(vl, vl, false, false);
  const auto h = __builtin_amdgcn_permlane16_swap(vh, vh, false, false);
  lo = __hiloint2double((int)h[0], (int)l[0]);
  hi = __hiloint2double((int)h[1], (int)l[1]);
}
template <int N, bool NEG>
__device__ inline double fmac_bc(double acc, double rep, double own) {
  if constexpr (NEG)
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(rep), "v"(own), "n"(N));
  else
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(rep), "v"(own), "n"(N));
  return acc;
}

// the accumulator and the second factor written by the two VALU instructions
// right before the fused FMA, no wait state in between (only the DPP source
// keeps its s_nop): the kernel's FMAs follow a v_mov of their accumulator or
// the previous FMA of the same accumulator back to back
template <int N>
__device__ inline double fmac_bc_tight(double acc, double rep, double own) {
  double g, o;
  asm volatile("s_nop 1\n\tv_mul_f64 %1, %4, 1.0\n\tv_mov_b64 %0, %3\n\t"
               "v_fmac_f64_dpp %0, %2, %1 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
               "v_fmac_f64_dpp %0, %2, %1 row_newbcast:%5 row_mask:0xf bank_mask:0xf"
               : "=&v"(g), "=&v"(o) : "v"(rep), "v"(acc), "v"(own), "n"(N));
  return g;
}

// ---- (1) values ----
constexpr int kSets = 8, kRaw = 32, kPath = 64, kTight = 16;  // per set: N x sign, s x sign, N back to back
constexpr int kCases = kRaw + kPath + kTight;
template <int C>
__device__ void value_cases(double val, double own, double acc, int lane, double* got, double* ref) {
  if constexpr (C < kCases) {
    double g, r;
    if constexpr (C < kRaw) {
      constexpr int N = C >> 1;
      constexpr bool NEG = C & 1;
      g = fmac_bc<N, NEG>(acc, val, own);
      const double b = __shfl(val, (lane & ~15) | N);
      r = fma(b, NEG ? -own : own, acc);
    } else if constexpr (C >= kRaw + kPath) {
      constexpr int N = C - kRaw - kPath;
      g = fmac_bc_tight<N>(acc, val, own);
      const double b = __shfl(val, (lane & ~15) | N);
      r = fma(b, own, fma(b, own, acc));
    } else {
      constexpr int S = (C - kRaw) >> 1;
      constexpr bool NEG = C & 1;
      double lo, hi;
      rep16(val, lo, hi);
      g = fmac_bc<(S & 15), NEG>(acc, S < 16 ? lo : hi, own);
      const double b = __shfl(val, (lane & 32) | S);
      r = fma(b, NEG ? -own : own, acc);
    }
    got[C * 64 + lane] = g;
    ref[C * 64 + lane] = r;
    value_cases<C + 1>(val, own, acc, lane, got, ref);
  }
}
__global__ void values_k(const double* in, double* got, double* ref, unsigned long long mask) {
  const int lane = threadIdx.x, set = blockIdx.x;
  const double val = in[(set * 3 + 0) * 64 + lane], own = in[(set * 3 + 1) * 64 + lane], acc = in[(set * 3 + 2) * 64 + lane];
  if ((mask >> lane) & 1) value_cases<0>(val, own, acc, lane, got + set * kCases * 64, ref + set * kCases * 64);
}

// ---- (2) cycles ----
constexpr int kOps = 256, kAcc = 16, kReps = 16;
// MODE 0: v_fmac_f64, 1: v_fmac_f64_dpp row_newbcast, 2: rep16 of one double, 3: ds_read_b128 + 2 FMAs
template <int MODE>
__global__ void cycles_k(unsigned long long* ticks, double* sink, double seed) {
  __shared__ double2 buf[128];
  const int t = threadIdx.x;
  if (t < 128) buf[t] = double2{seed + t, seed - t};
  double a[kAcc], b = seed * 0.5 + t, c = 1.0 + 1e-9 * t;
#pragma unroll
  for (int i = 0; i < kAcc; i++) a[i] = seed + i;
  __syncthreads();
  unsigned long long best = ~0ull;
  for (int rep = 0; rep < kReps; rep++) {
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (MODE == 0 || MODE == 1) {
#pragma unroll
      for (int k = 0; k < kOps / kAcc; k++)
#pragma unroll
        for (int i = 0; i < kAcc; i++) {
          if constexpr (MODE == 0) asm volatile("v_fmac_f64 %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
          else asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:5 row_mask:0xf bank_mask:0xf" : "+v"(a[i]) : "v"(b), "v"(c));
        }
    } else if constexpr (MODE == 2) {
#pragma unroll
      for (int k = 0; k < kOps / kAcc; k++)
#pragma unroll
        for (int i = 0; i < kAcc; i++) {
          double lo, hi;
          rep16(a[i], lo, hi);
          asm volatile("" : "+v"(lo), "+v"(hi));
          a[i] = (k & 1) ? lo : hi;
        }
    } else {
#pragma unroll
      for (int k = 0; k < kOps / kAcc; k++)
#pragma unroll
        for (int i = 0; i < kAcc / 2; i++) {
          const double2 v = buf[k * 8 + i];  // one address for the whole wave
          a[2 * i] = fma(v.x, c, a[2 * i]);
          a[2 * i + 1] = fma(v.y, c, a[2 * i + 1]);
        }
    }
    asm volatile("s_nop 0" ::: "memory");
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    best = t1 - t0 < best ? t1 - t0 : best;
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < kAcc; i++) s += a[i];
  sink[blockIdx.x * blockDim.x + t] = s;
  if ((t & 63) == 0) ticks[blockIdx.x * (blockDim.x / 64) + t / 64] = best;
}

static uint64_t bits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
static double from_bits(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double rnd_double() {  // sign, exponent within +-40 of 1.0, random mantissa
  const uint64_t r = rng();
  const uint64_t e = 1023 - 40 + (rng() % 81);
  return from_bits((r & 0x800FFFFFFFFFFFFFull) | (e << 52));
}
static double special(int kind) {
  const uint64_t r = rng();
  const uint64_t sign = r & 0x8000000000000000ull;
  switch (kind) {
    case 0: return from_bits(sign);                                            // +-0
    case 1: return from_bits(sign | (r & 0x000FFFFFFFFFFFFFull) | 1ull);        // denormal
    case 2: return from_bits(sign | 0x7FF0000000000000ull);                     // +-inf
    default: return from_bits(sign | 0x7FF8000000000000ull | (r & 0xFFFFull));  // quiet NaN with a payload
  }
}

template <int MODE>
static int run_cycles(const char* name, int waves_per_simd, unsigned long long* dticks, double* dsink, int blocks) {
  const int threads = 256 * waves_per_simd, waves = threads / 64;
  hipLaunchKernelGGL(cycles_k<MODE>, dim3(blocks), dim3(threads), 0, 0, dticks, dsink, 1.25);
  CK(hipDeviceSynchronize());
  std::vector<unsigned long long> h(blocks * waves);
  CK(hipMemcpy(h.data(), dticks, h.size() * 8, hipMemcpyDeviceToHost));
  std::sort(h.begin(), h.end());
  printf("%-44s %d wave(s)/SIMD: ticks per %d ops: min %llu median %llu max %llu -> %.2f per op (median)\n", name,
         waves_per_simd, kOps, h.front(), h[h.size() / 2], h.back(), (double)h[h.size() / 2] / kOps);
  return 0;
}

int main() {
  hipDeviceProp_t p;
  CK(hipGetDeviceProperties(&p, 0));
  printf("device %s arch %s CUs %d clock %d kHz\n", p.name, p.gcnArchName, p.multiProcessorCount, p.clockRate);
  // (1) values
  std::vector<double> in(kSets * 3 * 64);
  for (int s = 0; s < kSets; s++)
    for (int k = 0; k < 3; k++)
      for (int l = 0; l < 64; l++) {
        double v = rnd_double();
        if (s == 4) v = special(0);
        if (s == 5) v = (rng() & 1) ? special(1) : rnd_double();
        if (s == 6) v = (rng() % 3 == 0) ? special(2) : rnd_double();
        if (s == 7) v = (rng() & 1) ? special((int)(rng() % 4)) : rnd_double();
        in[(s * 3 + k) * 64 + l] = v;
      }
  const size_t nout = (size_t)kSets * kCases * 64;
  double *din, *dgot, *dref;
  CK(hipMalloc(&din, in.size() * 8));
  CK(hipMalloc(&dgot, nout * 8));
  CK(hipMalloc(&dref, nout * 8));
  CK(hipMemcpy(din, in.data(), in.size() * 8, hipMemcpyHostToDevice));
  const unsigned long long masks[3] = {~0ull, 0x00000000FFFFFFFFull, 0xFFFFFFFF00000000ull};
  const char* mname[3] = {"all 64 lanes", "lower half only", "upper half only"};
  const char* sname[kSets] = {"random", "random", "random", "random", "signed zeros", "denormals", "infinities", "mixed specials"};
  long total_bad = 0;
  for (int m = 0; m < 3; m++) {
    CK(hipMemset(dgot, 0x5a, nout * 8));
    CK(hipMemset(dref, 0x5a, nout * 8));
    hipLaunchKernelGGL(values_k, dim3(kSets), dim3(64), 0, 0, din, dgot, dref, masks[m]);
    CK(hipDeviceSynchronize());
    std::vector<double> got(nout), ref(nout);
    CK(hipMemcpy(got.data(), dgot, nout * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(ref.data(), dref, nout * 8, hipMemcpyDeviceToHost));
    for (int s = 0; s < kSets; s++) {
      long bad = 0, badh = 0, nanpay = 0, n = 0, untouched = 0;
      for (int c = 0; c < kCases; c++)
        for (int l = 0; l < 64; l++) {
          const size_t i = ((size_t)s * kCases + c) * 64 + l;
          if (!((masks[m] >> l) & 1)) {  // an inactive lane: nothing written
            untouched += bits(got[i]) != 0x5a5a5a5a5a5a5a5aull;
            continue;
          }
          n++;
          // the host's own fma of the same inputs
          const bool tight = c >= kRaw + kPath;
          const int srcl = tight ? ((l & ~15) | (c - kRaw - kPath)) : (c < kRaw) ? ((l & ~15) | (c >> 1)) : ((l & 32) | ((c - kRaw) >> 1));
          const double val = in[(s * 3) * 64 + srcl];
          const double own = in[(s * 3 + 1) * 64 + l], acc = in[(s * 3 + 2) * 64 + l];
          const double hr = tight ? std::fma(val, own, std::fma(val, own, acc)) : std::fma(val, (c & 1) ? -own : own, acc);
          if (std::isnan(got[i]) && std::isnan(ref[i])) {
            nanpay += bits(got[i]) != bits(ref[i]);
          } else {
            bad += bits(got[i]) != bits(ref[i]);
          }
          if (!(std::isnan(got[i]) && std::isnan(hr))) badh += bits(got[i]) != bits(hr);
        }
      printf("values, %-16s set %d (%-14s): %ld results, %ld differ from the device fma, %ld from the host fma, "
             "%ld NaN payloads differ, %ld inactive lanes written\n", mname[m], s, sname[s], n, bad, badh, nanpay, untouched);
      total_bad += bad + untouched;
    }
  }
  printf("values: %s (%ld mismatches; host-fma differences on denormals reflect the host's and the device's denormal modes only if any)\n",
         total_bad ? "FAIL" : "PASS", total_bad);
  // (2) cycles
  const int blocks = 8;
  unsigned long long* dticks;
  double* dsink;
  CK(hipMalloc(&dticks, blocks * 12 * 8));
  CK(hipMalloc(&dsink, blocks * 768 * 8));
  printf("cycles: s_memtime ticks around %d instructions per wave, best of %d repeats per wave, %d blocks\n", kOps, kReps, blocks);
  for (int w = 1; w <= 3; w += 2) {
    if (run_cycles<0>("v_fmac_f64", w, dticks, dsink, blocks)) return 1;
    if (run_cycles<1>("v_fmac_f64_dpp row_newbcast", w, dticks, dsink, blocks)) return 1;
    if (run_cycles<2>("rep16 of one double (2 v_mov + 2 swap)", w, dticks, dsink, blocks)) return 1;
    if (run_cycles<3>("ds_read_b128 (uniform) + 2 v_fma_f64, per 2 FMA", w, dticks, dsink, blocks)) return 1;
  }
  printf("(the ds_read_b128 row times %d reads and %d FMAs)\n", kOps / 2, kOps);
  return total_bad ? 2 : 0;
}
