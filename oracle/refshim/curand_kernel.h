/*
 * refshim/curand_kernel.h -- cuRAND's XORWOW generator as the reference uses
 * it: curandState, curand_init, curand, curand_uniform.  Test infrastructure.
 *
 *   state layout   curandStateXORWOW: d, v[5], the Box-Muller fields; 48 bytes
 *   curand_init    cuRAND's published seed scramble, then the 2^67-step
 *                  subsequence skip and the offset skip of rocRAND's host
 *                  engine (xorwow_rocrand.cpp), an implementation independent
 *                  of the oracle's
 *   curand         one step of the recurrence (rocRAND's engine)
 *   curand_uniform cuRAND's mapping x * 2^-32 + 2^-33 (rocRAND's differs:
 *                  2^-32 + x * 2^-32)
 */
#ifndef MORT_REFSHIM_CURAND_KERNEL_H
#define MORT_REFSHIM_CURAND_KERNEL_H

#include "cuda_runtime.h"

struct curandStateXORWOW {
    unsigned int d;
    unsigned int v[5];
    int boxmuller_flag;
    int boxmuller_flag_double;
    float boxmuller_extra;
    double boxmuller_extra_double;
};
typedef curandStateXORWOW curandStateXORWOW_t;
typedef curandStateXORWOW curandState_t;
typedef curandStateXORWOW curandState;
static_assert(sizeof(curandState) == 48, "cuRAND's XORWOW state is 48 bytes");

extern "C" void mort_refshim_xorwow_skip(unsigned int *d, unsigned int *v, unsigned long long subsequence,
                                         unsigned long long offset);
extern "C" unsigned int mort_refshim_xorwow_next(unsigned int *d, unsigned int *v);

inline void curand_init(unsigned long long seed, unsigned long long subsequence, unsigned long long offset,
                        curandState *state) {
    const unsigned int s0 = (unsigned int)seed ^ 0xaad26b49u;
    const unsigned int s1 = (unsigned int)(seed >> 32) ^ 0xf7dcefddu;
    const unsigned int t0 = 1099087573u * s0;
    const unsigned int t1 = 2591861531u * s1;
    state->d = 6615241u + t1 + t0;
    state->v[0] = 123456789u + t0;
    state->v[1] = 362436069u ^ t0;
    state->v[2] = 521288629u + t1;
    state->v[3] = 88675123u ^ t1;
    state->v[4] = 5783321u + t0;
    mort_refshim_xorwow_skip(&state->d, state->v, subsequence, offset);
    state->boxmuller_flag = 0;
    state->boxmuller_flag_double = 0;
    state->boxmuller_extra = 0.0f;
    state->boxmuller_extra_double = 0.0;
}

inline unsigned int curand(curandState *state) { return mort_refshim_xorwow_next(&state->d, state->v); }

/* 2.3283064e-10f is 2^-32 exactly: the product is exact */
inline float curand_uniform(curandState *state) { return curand(state) * 2.3283064e-10f + (2.3283064e-10f / 2.0f); }

#endif /* MORT_REFSHIM_CURAND_KERNEL_H */
