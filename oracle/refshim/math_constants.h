/* refshim/math_constants.h -- the two CUDA math constants the reference's
 * device code uses, with CUDA's values (fp32 infinity and pi). */
#ifndef MORT_REFSHIM_MATH_CONSTANTS_H
#define MORT_REFSHIM_MATH_CONSTANTS_H
#define CUDART_INF_F __builtin_huge_valf()
#define CUDART_PI_F 3.141592654f
#endif
