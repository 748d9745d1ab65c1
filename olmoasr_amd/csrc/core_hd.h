// OASR_HD: what every function of a *_core.h rule is declared with, so that one text compiles into the device kernel (under hipcc) and into
// the plain C++ host twin and host check alike.
#pragma once

#if defined(__HIPCC__)
#define OASR_HD __host__ __device__ __forceinline__
#else
#define OASR_HD inline
#endif
