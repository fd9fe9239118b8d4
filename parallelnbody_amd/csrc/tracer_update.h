// The update of a massless tracer behind its acceleration — OctreeSearch.cpp:29-30 as the bodies get it: v = v + dt*a; x = x + dt*v in
// fp32 with multiply and add kept apart (FVector's operators, no FMA).  One copy for the two kernels that move tracers
// (probe_fold_kernel at theta = 0, bh_probe_walk_kernel at theta > 0): their bits must be the same function of (y, v, a, dt).
#pragma once
#include <hip/hip_runtime.h>

namespace nbody {

__device__ __forceinline__ void tracer_kick_drift(float dt, float ax, float ay, float az, float4 &v, float4 &x) {
#pragma clang fp contract(off)
  const float kx = dt * ax, ky = dt * ay, kz = dt * az;
  v.x = v.x + kx; v.y = v.y + ky; v.z = v.z + kz;
  const float dx = dt * v.x, dy = dt * v.y, dz = dt * v.z;
  x.x = x.x + dx; x.y = x.y + dy; x.z = x.z + dz;
}

}  // namespace nbody
