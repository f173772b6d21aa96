// tone_device.h -- the tone steps pbr_head.hip and display.hip share. Both files are built with
// -ffp-contract=off and include these definitions as they stand, so a tone computed by either has the same bits.
#pragma once

namespace r3dg {

// a NaN stays a NaN, as through torch.clamp (fminf / fmaxf would drop it)
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// utils/graphics_utils.py:197-201 hdr2ldr, its Python constants rounded to float32 where they meet the tensor
__device__ __forceinline__ float aces(float x) {
    const float s = x * 0.666667f;
    return (s * (2.51f * s + 0.03f)) / (s * (2.43f * s + 0.59f) + 0.14f);
}

}  // namespace r3dg
