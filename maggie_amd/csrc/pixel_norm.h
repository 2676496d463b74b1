// The two fp32 forms of a uint8 pixel on the input side, shared by preprocess.hip and geometry.hip so that the kernels cannot drift apart.
// IEEE divisions, operation for operation the reference's arithmetic (transforms.py:777-782, him.py:157-158): bit-exact.
#pragma once
#include <hip/hip_runtime.h>

// ToTensor + Normalize.norm: (v / 255 - mean) / std
__device__ __forceinline__ float mg_norm_u8(int v, float mean, float std) { return __fdiv_rn(__fdiv_rn((float)v, 255.0f) - mean, std); }
// the same on a pixel that is already a float (the channel shift of RandomAffine leaves non-integer values): (f / 255 - mean) / std
__device__ __forceinline__ float mg_norm_f32(float f, float mean, float std) { return __fdiv_rn(__fdiv_rn(f, 255.0f) - mean, std); }
// alpha / mask planes: v / 255, 0 below `thresh`
__device__ __forceinline__ float mg_scale_u8(int v, int thresh) { return v < thresh ? 0.f : __fdiv_rn((float)v, 255.0f); }
