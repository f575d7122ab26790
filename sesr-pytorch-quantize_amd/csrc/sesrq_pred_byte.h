// The byte of a prediction, as every export of the project forms it (the reference's PNG export, sim.py): an int8 output is first
// dequantised as sesrq_forward forms out_f, then u = trunc(fl32(clip(p, 0, 1) * 255)).  The rounding intrinsics are the definition.
// Device code with internal linkage; the libraries that include it stay libraries of their own.
#pragma once

#include <hip/hip_runtime.h>

namespace sesrq_pred {

// fl32((q - zero) * scale) of an int8 code q in the output domain (scale, zero)
__device__ inline float dequant(int q, int zero, float scale) { return __fmul_rn((float)(q - zero), scale); }

// u = trunc(fl32(clip(p, 0, 1) * 255)); a NaN gives 0
__device__ inline unsigned to_byte(float p) { return (unsigned)__fmul_rn(fminf(fmaxf(p, 0.f), 1.f), 255.f); }

}  // namespace sesrq_pred
