// O(N) bulk diagnostics of the owned bodies — nbody_get_moments and nbody_mass_within (include/nbody.h): streaming reductions over
// posm / vel / acc, 48 B a body on fp32 state and 96 B on fp64 state, every term and every sum in fp64.
//
// Geometry — a function of the owned count n alone (moments_geometry): neither the CU count, nor the precision, nor the radii.
//   slots  S   = min(kMomentSlotCap, ceil(n / 256))          kMomentSlotCap = 1024: four workgroups for each of the 256 CUs
//   run    per = ceil(n / S)                                 bodies per workgroup, contiguous: workgroup b owns [b per, min((b + 1) per, n))
//   launched   = ceil(n / per)  (<= S)                       no workgroup is idle
// Up to n = 262144 a workgroup's run is one trip of at most 256 bodies; beyond, the 1024 slots stay and the runs grow (n = 2^23: 8192
// bodies, 32 trips).  Lane t of a workgroup meets bodies lo + t, lo + t + 256, ... of its run, one 16-byte (fp64: 32-byte) load per
// array and trip, and adds their terms to its own fp64 accumulators in that order.
//
// Order of every sum, fixed by n: a lane's trips in order; the 64 lanes of a wave by the __shfl_xor tree 32, 16, ... 1 (energy_kernel's);
// the four waves in wave order, through LDS, into the workgroup's slot; then ONE workgroup (moments_fold_kernel, mass_within_fold_kernel) adds the slots of a value:
// lane l of the wave that owns the value adds slots l, l + 64, ... in order, the same tree joins the 64 lanes.  No atomics, nothing to
// clear beforehand: every slot that is read has been written by the launch before.  The same state gives the same bits on every call and
// on every device.
#include "../../include/nbody.h"
#include "kernels.h"
#include "pk_common.h"

namespace nbody {

namespace {

template <typename T> struct V4;
template <> struct V4<float> { using type = float4; };
template <> struct V4<double> { using type = double4; };

template <typename S> __device__ __forceinline__ S wave_sum(S v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// radii^2 of one nbody_mass_within call, a kernel argument
struct Radii2 { double v[kMassWithinMax]; };

// slot[24] of workgroup blockIdx.x, in the field order of nbody_moments: mass, mx[3], p[3], l[3], second[6], kinetic, virial, force[3],
// torque[3].  Products of fp32 state widened to double are exact; the terms of fp64 state round as the expressions below say (the
// compiler may fuse a product into the add that follows it).
template <typename T>
__global__ __launch_bounds__(kBlock) void moments_kernel(const typename V4<T>::type *__restrict__ posm,
                                                         const typename V4<T>::type *__restrict__ vel,
                                                         const typename V4<T>::type *__restrict__ acc, int i_begin, int i_count,
                                                         int per, double *__restrict__ part) {
  using V = typename V4<T>::type;
  __shared__ double red[kBlock / 64][kMomentValues];
  const int t = threadIdx.x;
  const long long lo64 = (long long)blockIdx.x * per;
  const int lo = (int)lo64, hi = (int)min(lo64 + per, (long long)i_count);
  double s[kMomentValues];
#pragma unroll
  for (int k = 0; k < kMomentValues; ++k) s[k] = 0.0;
  for (int i = lo + t; i < hi; i += kBlock) {
    const V pm = posm[i_begin + i], vv = vel[i], aa = acc[i];
    const double x = pm.x, y = pm.y, z = pm.z, m = pm.w;
    const double vx = vv.x, vy = vv.y, vz = vv.z;
    const double ax = aa.x, ay = aa.y, az = aa.z;
    s[0] += m;
    s[1] += m * x; s[2] += m * y; s[3] += m * z;
    s[4] += m * vx; s[5] += m * vy; s[6] += m * vz;
    s[7] += m * (y * vz - z * vy); s[8] += m * (z * vx - x * vz); s[9] += m * (x * vy - y * vx);
    s[10] += m * (x * x); s[11] += m * (y * y); s[12] += m * (z * z);
    s[13] += m * (x * y); s[14] += m * (x * z); s[15] += m * (y * z);
    s[16] += 0.5 * m * ((vx * vx + vy * vy) + vz * vz);
    s[17] += m * ((x * ax + y * ay) + z * az);
    s[18] += m * ax; s[19] += m * ay; s[20] += m * az;
    s[21] += m * (y * az - z * ay); s[22] += m * (z * ax - x * az); s[23] += m * (x * ay - y * ax);
  }
#pragma unroll
  for (int k = 0; k < kMomentValues; ++k) {
    const double w = wave_sum(s[k]);
    if ((t & 63) == 0) red[t >> 6][k] = w;
  }
  __syncthreads();
  if (t < kMomentValues) {
    double v = red[0][t];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) v += red[w][t];
    part[(size_t)blockIdx.x * kMomentValues + t] = v;
  }
}

// sum over the slots of part[slot * stride + v] for the calling wave's value v: lane l adds slots l, l + 64, ... in order, the shuffle
// tree joins the lanes (every lane returns the sum)
template <typename S> __device__ __forceinline__ S fold_slots(const S *__restrict__ part, int stride, int v, int slots) {
  S s = 0;
  for (int q = threadIdx.x & 63; q < slots; q += 64) s += part[(size_t)q * stride + v];
  return wave_sum(s);
}

// out[v] = the slots' sum of value v; wave w owns the values w, w + 4, ...
__global__ __launch_bounds__(kBlock) void moments_fold_kernel(const double *__restrict__ part, int slots, double *__restrict__ out) {
  for (int v = threadIdx.x >> 6; v < kMomentValues; v += kBlock / 64) {
    const double s = fold_slots(part, kMomentValues, v, slots);
    if ((threadIdx.x & 63) == 0) out[v] = s;
  }
}

// the same for the k radii of nbody_mass_within: masses and counts
__global__ __launch_bounds__(kBlock) void mass_within_fold_kernel(const double *__restrict__ part_m, const long long *__restrict__ part_c,
                                                                  int k, int slots, double *__restrict__ out_m,
                                                                  long long *__restrict__ out_c) {
  for (int v = threadIdx.x >> 6; v < k; v += kBlock / 64) {
    const double m = fold_slots(part_m, kMassWithinMax, v, slots);
    const long long c = fold_slots(part_c, kMassWithinMax, v, slots);
    if ((threadIdx.x & 63) == 0) { out_m[v] = m; out_c[v] = c; }
  }
}

// Per radius q < k: mass[q] = sum of the masses of the run's bodies with d2 <= r2[q], cnt[q] = their number.  A body is loaded once and
// tested against every radius; KMAX (>= k) accumulator pairs live in registers.  d2 is formed without contraction, so that membership
// is the plain C expression's: dx = (double)x - cx; d2 = (dx*dx + dy*dy) + dz*dz; inside iff d2 <= r*r.
template <typename T, int KMAX>
__global__ __launch_bounds__(kBlock) void mass_within_kernel(const typename V4<T>::type *__restrict__ posm, int i_begin, int i_count,
                                                             int per, double cx, double cy, double cz, Radii2 radii2, int k,
                                                             double *__restrict__ part_m, long long *__restrict__ part_c) {
#pragma clang fp contract(off)
  using V = typename V4<T>::type;
  __shared__ double r2[kMassWithinMax];
  __shared__ double red_m[kBlock / 64][kMassWithinMax];
  __shared__ int red_c[kBlock / 64][kMassWithinMax];
  const int t = threadIdx.x;
  if (t < kMassWithinMax) r2[t] = radii2.v[t];
  __syncthreads();
  const long long lo64 = (long long)blockIdx.x * per;
  const int lo = (int)lo64, hi = (int)min(lo64 + per, (long long)i_count);
  double ms[KMAX];
  int cs[KMAX];
#pragma unroll
  for (int q = 0; q < KMAX; ++q) { ms[q] = 0.0; cs[q] = 0; }
  for (int i = lo + t; i < hi; i += kBlock) {
    const V pm = posm[i_begin + i];
    const double dx = (double)pm.x - cx, dy = (double)pm.y - cy, dz = (double)pm.z - cz;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const double m = pm.w;
#pragma unroll
    for (int q = 0; q < KMAX; ++q) {
      if (q < k) {                                   // (uniform: k is a kernel argument)
        const bool in = d2 <= r2[q];
        ms[q] += in ? m : 0.0;
        cs[q] += in ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < KMAX; ++q) {
    if (q < k) {
      const double wm = wave_sum(ms[q]);
      const int wc = wave_sum(cs[q]);
      if ((t & 63) == 0) { red_m[t >> 6][q] = wm; red_c[t >> 6][q] = wc; }
    }
  }
  __syncthreads();
  if (t < k) {
    double m = red_m[0][t];
    long long c = red_c[0][t];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) { m += red_m[w][t]; c += red_c[w][t]; }
    part_m[(size_t)blockIdx.x * kMassWithinMax + t] = m;
    part_c[(size_t)blockIdx.x * kMassWithinMax + t] = c;
  }
}

}  // namespace

void moments_geometry(int i_count, int *slots, int *per) {
  const int n = i_count > 0 ? i_count : 1;
  const int blocks = (n + kBlock - 1) / kBlock;
  const int cap = blocks < kMomentSlotCap ? blocks : kMomentSlotCap;
  *per = (n + cap - 1) / cap;
  *slots = (n + *per - 1) / *per;
}

size_t moments_scratch_bytes(int i_count) {
  int slots, per;
  moments_geometry(i_count, &slots, &per);
  // the results (kMassWithinMax doubles — the 24 moments fit them — and kMassWithinMax counts), then the slots' doubles and counts
  return (size_t)(2 + 2 * (size_t)slots) * kMassWithinMax * 8;
}

hipError_t launch_moments(int precision, const void *posm, const void *vel, const void *acc, int i_begin, int i_count, void *scratch,
                          hipStream_t s) {
  int slots, per;
  moments_geometry(i_count, &slots, &per);
  double *out = (double *)scratch, *part = out + 2 * kMassWithinMax;
  if (precision == NBODY_PREC_F64)
    hipLaunchKernelGGL((moments_kernel<double>), dim3(slots), dim3(kBlock), 0, s, (const double4 *)posm, (const double4 *)vel,
                       (const double4 *)acc, i_begin, i_count, per, part);
  else
    hipLaunchKernelGGL((moments_kernel<float>), dim3(slots), dim3(kBlock), 0, s, (const float4 *)posm, (const float4 *)vel,
                       (const float4 *)acc, i_begin, i_count, per, part);
  hipLaunchKernelGGL(moments_fold_kernel, dim3(1), dim3(kBlock), 0, s, (const double *)part, slots, out);
  return hipGetLastError();
}

hipError_t launch_mass_within(int precision, const void *posm, int i_begin, int i_count, const double centre[3], const double *radii,
                              int k, void *scratch, hipStream_t s) {
  int slots, per;
  moments_geometry(i_count, &slots, &per);
  double *out_m = (double *)scratch;
  long long *out_c = (long long *)(out_m + kMassWithinMax);
  double *part_m = out_m + 2 * kMassWithinMax;
  long long *part_c = (long long *)(part_m + (size_t)slots * kMassWithinMax);
  Radii2 r2;
  for (int q = 0; q < kMassWithinMax; ++q) r2.v[q] = q < k ? radii[q] * radii[q] : 0.0;   // the threshold: one fp64 multiply
#define NBODY_LAUNCH_MW(T, V, KMAX)                                                                                                  \
  hipLaunchKernelGGL((mass_within_kernel<T, KMAX>), dim3(slots), dim3(kBlock), 0, s, (const V *)posm, i_begin, i_count, per, centre[0], \
                     centre[1], centre[2], r2, k, part_m, part_c)
  // (two register budgets for the accumulators; a radius' sums are formed in the same order by either)
  if (precision == NBODY_PREC_F64) { if (k <= 16) NBODY_LAUNCH_MW(double, double4, 16); else NBODY_LAUNCH_MW(double, double4, kMassWithinMax); }
  else { if (k <= 16) NBODY_LAUNCH_MW(float, float4, 16); else NBODY_LAUNCH_MW(float, float4, kMassWithinMax); }
#undef NBODY_LAUNCH_MW
  hipLaunchKernelGGL(mass_within_fold_kernel, dim3(1), dim3(kBlock), 0, s, (const double *)part_m, (const long long *)part_c, k, slots,
                     out_m, out_c);
  return hipGetLastError();
}

}  // namespace nbody
