// K14: SchNet's shifted softplus (PyG ShiftedSoftplus: softplus(x) - log 2, applied to the
// (E, 128) filter-network hidden layer, schnet.py:72 via CFConv's nn, and to node features).
// torch.nn.functional.softplus semantics (beta 1, threshold 20):
//   forward : y = (x > 20 ? x : log1p(exp(x))) - shift
//   backward: dx = x > 20 ? g : g * sigmoid(x)
// One float4 per thread, grid-stride: one read + one write pass (the library path ran the
// softplus and the shift subtraction as separate passes).
#include "gmp_common.h"

namespace gmp {
namespace {

// softplus(x) = max(x, 0) + log(1 + exp(-|x|)) with the native exp / log (absolute error
// ~1e-7: 1 + exp(-|x|) lies in [1, 2]); for x > 20 the correction is below half an ulp of x, so
// torch's threshold-20 identity branch comes out the same.  r01's log1pf(expf(x)) form ran at
// 2.4 TB/s, limited by the accurate library calls.
__device__ __forceinline__ float ssp1(float x, float shift) {
  return (fmaxf(x, 0.f) + __logf(1.f + __expf(-fabsf(x)))) - shift;
}

// d softplus = sigmoid(x) = 1 / (1 + exp(-x)) (exp(-x) = inf for x << 0 gives 0)
__device__ __forceinline__ float ssp1_bwd(float x, float g) {
  return g / (1.f + __expf(-x));
}

__global__ __launch_bounds__(256) void ssp_fwd(const float4* __restrict__ x, int64_t n4,
                                               float shift, float4* __restrict__ y) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n4;
       t += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = x[t];
    y[t] = make_float4(ssp1(v.x, shift), ssp1(v.y, shift), ssp1(v.z, shift), ssp1(v.w, shift));
  }
}

__global__ __launch_bounds__(256) void ssp_bwd(const float4* __restrict__ x,
                                               const float4* __restrict__ g, int64_t n4,
                                               float4* __restrict__ dx) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n4;
       t += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = x[t], w = g[t];
    dx[t] = make_float4(ssp1_bwd(v.x, w.x), ssp1_bwd(v.y, w.y), ssp1_bwd(v.z, w.z),
                        ssp1_bwd(v.w, w.w));
  }
}

// Second order: the backward dx = g * sigmoid(x) differentiated once more.  With the cotangent a
// of dx:  gg = a * sigmoid(x) (the same form as ssp1_bwd) and gx = a * g * sigmoid'(x), where
// sigmoid'(x) = e / (1 + e)^2 with e = exp(-|x|) in (0, 1]: no overflow, and it underflows to 0
// for large |x| (finite everywhere).
__device__ __forceinline__ void ssp1_bwd2(float x, float g, float a, float& gg, float& gx) {
  gg = a / (1.f + __expf(-x));
  const float e = __expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  gx = a * g * (e * r * r);
}

__global__ __launch_bounds__(256) void ssp_bwd2(const float4* __restrict__ x,
                                                const float4* __restrict__ g,
                                                const float4* __restrict__ a, int64_t n4,
                                                float4* __restrict__ gg, float4* __restrict__ gx) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n4;
       t += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = x[t], w = g[t], c = a[t];
    float4 og, ox;
    ssp1_bwd2(v.x, w.x, c.x, og.x, ox.x);
    ssp1_bwd2(v.y, w.y, c.y, og.y, ox.y);
    ssp1_bwd2(v.z, w.z, c.z, og.z, ox.z);
    ssp1_bwd2(v.w, w.w, c.w, og.w, ox.w);
    gg[t] = og;
    gx[t] = ox;
  }
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

unsigned grid_for4(int64_t n4) {
  return (unsigned)std::min<int64_t>(ceil_div(n4, 256), 256 * 32);
}

}  // namespace
}  // namespace gmp

using namespace gmp;

extern "C" {

int gmp_ssp_fwd_f32(const float* x, int64_t n, float shift, float* y, void* stream) {
  GMP_CHECK_ARG(n >= 0);
  if (n == 0) return GMP_OK;
  GMP_CHECK_ARG(x && y && n % 4 == 0 && aligned16(x) && aligned16(y));
  ssp_fwd<<<grid_for4(n / 4), 256, 0, as_stream(stream)>>>(
      reinterpret_cast<const float4*>(x), n / 4, shift, reinterpret_cast<float4*>(y));
  return launch_status();
}

int gmp_ssp_bwd_f32(const float* x, const float* grad_y, int64_t n, float* grad_x,
                    void* stream) {
  GMP_CHECK_ARG(n >= 0);
  if (n == 0) return GMP_OK;
  GMP_CHECK_ARG(x && grad_y && grad_x && n % 4 == 0 && aligned16(x) && aligned16(grad_y) &&
                aligned16(grad_x));
  ssp_bwd<<<grid_for4(n / 4), 256, 0, as_stream(stream)>>>(
      reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(grad_y), n / 4,
      reinterpret_cast<float4*>(grad_x));
  return launch_status();
}

int gmp_ssp_bwd2_f32(const float* x, const float* grad_y, const float* a, int64_t n, float* gg,
                     float* gx, void* stream) {
  GMP_CHECK_ARG(n >= 0);
  if (n == 0) return GMP_OK;
  GMP_CHECK_ARG(x && grad_y && a && gg && gx && n % 4 == 0 && aligned16(x) &&
                aligned16(grad_y) && aligned16(a) && aligned16(gg) && aligned16(gx));
  ssp_bwd2<<<grid_for4(n / 4), 256, 0, as_stream(stream)>>>(
      reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(grad_y),
      reinterpret_cast<const float4*>(a), n / 4, reinterpret_cast<float4*>(gg),
      reinterpret_cast<float4*>(gx));
  return launch_status();
}

}  // extern "C"
