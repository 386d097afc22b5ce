// What the host+device texts (optim_math.h, data_math.h, bn_math.h: one spelling for a gfx950
// kernel and its CPU twin, cpu_ref.cpp being plain C++) share: DDLPC_HD and fp32 operations that
// round on their own.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DDLPC_HD __host__ __device__
#else
#define DDLPC_HD
#endif
#define DDLPC_HDI DDLPC_HD __attribute__((always_inline)) inline   // as DDLPC_DEVICE (common.h)

namespace ddlpc {

// Device: the intrinsics, and for the multiply an asm (HIP's __fmul_rn is a plain operator that
// the default -ffp-contract=fast still fuses into a following add).  Host: contraction off.
#if defined(__HIP_DEVICE_COMPILE__)
DDLPC_HDI float add_rn(float a, float b) { return __fadd_rn(a, b); }
DDLPC_HDI float sub_rn(float a, float b) { return __fsub_rn(a, b); }
DDLPC_HDI float div_rn(float a, float b) { return __fdiv_rn(a, b); }
DDLPC_HDI float mul_rn(float a, float b) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
#else
DDLPC_HDI float div_rn(float a, float b) { return a / b; }
DDLPC_HDI float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
DDLPC_HDI float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
DDLPC_HDI float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
#endif

}  // namespace ddlpc
