// One element of FocalLoss_BCE_2d (tools/losses/focal_loss.py:255-301): the loss term and its gradient from (pred, target).
// Shared by caller.hip (every element) and topk_loss.hip (the selected elements), so that both form the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace unetpp {

// -> the loss term l; g = (dl/dp / rows) * scale (scale: 1 for a single head, 1 / heads under the trainer's mean over
// heads -- a second float32 product, as autograd forms it).  cube: gamma == 3.
// kLow: gamma < 1, where u^(gamma-1) is inf at u == 0 (an exact hit, or |p - t| below float32 rounding of 1): there
// u^gamma is 0^0 = 1 for gamma == 0 (torch's value) and 0 otherwise, and gamma u^(gamma-1) log e is taken at its limit 0,
// so the loss stays finite and the gradient at an exact hit is 0.  gamma >= 1 runs the instantiation without the test.
template <bool kLow>
__device__ __forceinline__ float focal_element(float p, float t, float gamma, bool cube, float inv_rows, float scale,
                                               float& g) {
  const float d = p - t;
  const float err = (1.f - fabsf(d)) + 1e-20f;
  const float u = 1.f - err;
  const float lg = logf(err);
  const float ug1 = cube ? u * u : powf(u, gamma - 1.f);  // u^(gamma-1)
  const float ug = ug1 * u;
  float le = -ug * lg;
  float dl_de = gamma * ug1 * lg - ug / err;
  if constexpr (kLow) {
    if (u == 0.f) {
      le = 0.f;
      dl_de = (gamma == 0.f) ? -1.f / err : 0.f;
    }
  }
  const float sgn = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);
  g = (-dl_de * sgn * inv_rows) * scale;
  return le;
}

}  // namespace unetpp
