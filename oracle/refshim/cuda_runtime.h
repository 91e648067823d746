/*
 * refshim/cuda_runtime.h -- the part of the CUDA runtime that the reference's
 * device headers use, implemented for a plain C++ host build so that their
 * arithmetic runs on the CPU (oracle/ref_render.cpp).  Test infrastructure
 * only.  Written from CUDA's published semantics; nothing here is taken from
 * the reference.
 *
 *   qualifiers        __host__ __device__ __global__ __constant__ -> nothing
 *   launch geometry   threadIdx / blockIdx / blockDim: thread-local dim3s the
 *                     driver sets before it calls device code
 *   memory            cudaMalloc / cudaMemcpy / cudaMemcpyToSymbol -> host
 *   textures          pitch-2D tex2D<T> under a zeroed cudaTextureDesc
 *   math overloads    CUDA's float overloads of the <cmath> names, its mixed
 *                     min / max and pow(float, int).  MORT_REF_PINNED=1
 *                     ("pinned") sends sinf cosf acosf atan2f logf and fp64
 *                     sin / cos to include/mort_math.h, as the oracle and the
 *                     kernels do; MORT_REF_PINNED=0 ("native") to glibc
 *   host rand()       MSVC's rand(), RAND_MAX 0x7fff
 */
#ifndef MORT_REFSHIM_CUDA_RUNTIME_H
#define MORT_REFSHIM_CUDA_RUNTIME_H

/* Every system header the reference headers include comes first: the macros
 * below must not reach the standard library's own code. */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <limits>
#include <memory>
#include <string>
#include <vector>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "mort_math.h"

#ifndef MORT_REF_PINNED
#define MORT_REF_PINNED 1
#endif

#define __host__
#define __device__
#define __global__
#define __constant__
#define __shared__
#define __forceinline__ inline

/* ---- launch geometry ---- */
struct dim3 {
    unsigned int x = 0, y = 0, z = 0;
};
inline thread_local dim3 threadIdx, blockIdx, blockDim;

struct uchar4 {
    unsigned char x, y, z, w;
};

/* ---- errors and memory ---- */
typedef int cudaError_t;
#define cudaSuccess 0
enum cudaMemcpyKind { cudaMemcpyHostToHost = 0, cudaMemcpyHostToDevice = 1, cudaMemcpyDeviceToHost = 2,
                      cudaMemcpyDeviceToDevice = 3, cudaMemcpyDefault = 4 };

template <class T>
inline cudaError_t cudaMemcpyToSymbol(T &symbol, const void *src, size_t count, size_t offset = 0,
                                      cudaMemcpyKind kind = cudaMemcpyHostToDevice) {
    (void)kind;
    if (offset > sizeof(symbol) || count > sizeof(symbol) - offset) return 1;
    if (count) memcpy(reinterpret_cast<char *>(&symbol) + offset, src, count);
    return cudaSuccess;
}
inline cudaError_t cudaMalloc(void **p, size_t n) { *p = malloc(n ? n : 1); return *p ? cudaSuccess : 2; }
inline cudaError_t cudaFree(void *p) { free(p); return cudaSuccess; }
inline cudaError_t cudaMemcpy(void *dst, const void *src, size_t n, cudaMemcpyKind kind) {
    (void)kind;
    if (n) memcpy(dst, src, n);
    return cudaSuccess;
}

struct cudaDeviceProp {
    size_t texturePitchAlignment;
};
inline cudaError_t cudaGetDeviceProperties(cudaDeviceProp *prop, int device) {
    (void)device;
    prop->texturePitchAlignment = 32;
    return cudaSuccess;
}

/* ---- pitch-2D textures.  A zeroed cudaTextureDesc means unnormalised
 * coordinates, point filtering, element reads and an address mode that, for
 * unnormalised coordinates, clamps: tex2D<T>(obj, x, y) reads element
 * (clamp(floor(x), 0, width-1), clamp(floor(y), 0, height-1)), the width
 * counted in elements. ---- */
typedef unsigned long long cudaTextureObject_t;
enum cudaResourceType { cudaResourceTypeArray = 0, cudaResourceTypeMipmappedArray = 1, cudaResourceTypeLinear = 2,
                        cudaResourceTypePitch2D = 3 };
struct cudaChannelFormatDesc {
    int x, y, z, w;
    int f;
};
template <class T>
inline cudaChannelFormatDesc cudaCreateChannelDesc() {
    cudaChannelFormatDesc d = {int(8 * sizeof(T)), 0, 0, 0, 1};
    return d;
}
struct cudaResourceDesc {
    cudaResourceType resType;
    union {
        struct {
            void *devPtr;
            cudaChannelFormatDesc desc;
            size_t width;
            size_t height;
            size_t pitchInBytes;
        } pitch2D;
        char pad[64];
    } res;
};
struct cudaTextureDesc {
    int addressMode[3];
    int filterMode;
    int readMode;
    int sRGB;
    float borderColor[4];
    int normalizedCoords;
    unsigned int maxAnisotropy;
    int mipmapFilterMode;
    float mipmapLevelBias, minMipmapLevelClamp, maxMipmapLevelClamp;
};

struct mort_refshim_texture {
    const unsigned char *data;
    size_t width, height, pitch;
};

inline cudaError_t cudaCreateTextureObject(cudaTextureObject_t *obj, const cudaResourceDesc *res,
                                           const cudaTextureDesc *tex, const void *view) {
    (void)view;
    if (res->resType != cudaResourceTypePitch2D || tex->normalizedCoords || tex->filterMode || tex->readMode ||
        res->res.pitch2D.width == 0 || res->res.pitch2D.height == 0)
        return 3;
    mort_refshim_texture *t = new mort_refshim_texture;
    t->data = static_cast<const unsigned char *>(res->res.pitch2D.devPtr);
    t->width = res->res.pitch2D.width;
    t->height = res->res.pitch2D.height;
    t->pitch = res->res.pitch2D.pitchInBytes;
    *obj = reinterpret_cast<cudaTextureObject_t>(t);
    return cudaSuccess;
}
inline cudaError_t cudaDestroyTextureObject(cudaTextureObject_t obj) {
    delete reinterpret_cast<mort_refshim_texture *>(obj);
    return cudaSuccess;
}

template <class T>
inline T tex2D(cudaTextureObject_t obj, float x, float y) {
    const mort_refshim_texture *t = reinterpret_cast<const mort_refshim_texture *>(obj);
    const float fx = floorf(x), fy = floorf(y);
    /* clamp as floats: a NaN or huge coordinate never reaches an int conversion */
    const float mx = float(t->width - 1), my = float(t->height - 1);
    const size_t i = (fx >= 0.0f) ? size_t(fx < mx ? fx : mx) : 0;
    const size_t j = (fy >= 0.0f) ? size_t(fy < my ? fy : my) : 0;
    return *reinterpret_cast<const T *>(t->data + j * t->pitch + i * sizeof(T));
}

/* ---- CUDA's math overloads.  CUDA declares float versions of the <cmath>
 * names in the global namespace, so an unqualified sqrt(float) is sqrtf.  For
 * the IEEE-exact functions the standard library's std:: overloads are the
 * same functions. ---- */
using std::ceil;
using std::exp;
using std::fabs;
using std::floor;
using std::fmax;
using std::fmin;
using std::sqrt;
using std::tan;
using std::trunc;

/* min / max (CUDA math_functions): same-type floating point versions are
 * fminf / fmin; a float mixed with a double is widened and goes to fmin /
 * fmax in double */
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline unsigned int min(unsigned int a, unsigned int b) { return a < b ? a : b; }
inline unsigned int max(unsigned int a, unsigned int b) { return a > b ? a : b; }
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline double min(double a, double b) { return ::fmin(a, b); }
inline double max(double a, double b) { return ::fmax(a, b); }
inline double min(float a, double b) { return ::fmin(double(a), b); }
inline double min(double a, float b) { return ::fmin(a, double(b)); }
inline double max(float a, double b) { return ::fmax(double(a), b); }
inline double max(double a, float b) { return ::fmax(a, double(b)); }

/* pow(float, int): CUDA's fp32 overload multiplies by squaring (n = 5:
 * a * (a^2)^2); std::pow(float, int) computes in double and rounds once. */
inline float pow(float a, int n) {
    unsigned int e = n < 0 ? 0u - unsigned(n) : unsigned(n);
    float r = 1.0f;
    for (;;) {
        if (e & 1u) r = r * a;
        e >>= 1;
        if (e == 0) return n < 0 ? 1.0f / r : r;
        a = a * a;
    }
}
using std::pow;

/* The transcendental functions.  Unqualified calls resolve by argument type
 * as CUDA's overloads do; what computes them depends on the mode. */
#if MORT_REF_PINNED
inline float mort_refshim_sinf(float x) { return mort_sinf(x); }
inline float mort_refshim_cosf(float x) { return mort_cosf(x); }
inline float mort_refshim_acosf(float x) { return mort_acosf(x); }
inline float mort_refshim_atan2f(float y, float x) { return mort_atan2f(y, x); }
inline float mort_refshim_logf(float x) { return mort_logf(x); }
inline double mort_refshim_sind(double x) { return mort_sin(x); }
inline double mort_refshim_cosd(double x) { return mort_cos(x); }
#else
inline float mort_refshim_sinf(float x) { return ::sinf(x); }
inline float mort_refshim_cosf(float x) { return ::cosf(x); }
inline float mort_refshim_acosf(float x) { return ::acosf(x); }
inline float mort_refshim_atan2f(float y, float x) { return ::atan2f(y, x); }
inline float mort_refshim_logf(float x) { return ::logf(x); }
inline double mort_refshim_sind(double x) { return ::sin(x); }
inline double mort_refshim_cosd(double x) { return ::cos(x); }
#endif
inline float mort_refshim_sin(float x) { return mort_refshim_sinf(x); }
inline double mort_refshim_sin(double x) { return mort_refshim_sind(x); }
inline float mort_refshim_cos(float x) { return mort_refshim_cosf(x); }
inline double mort_refshim_cos(double x) { return mort_refshim_cosd(x); }
inline float mort_refshim_acos(float x) { return mort_refshim_acosf(x); }
inline double mort_refshim_acos(double x) { return ::acos(x); }
inline float mort_refshim_atan2(float y, float x) { return mort_refshim_atan2f(y, x); }
inline double mort_refshim_atan2(double y, double x) { return ::atan2(y, x); }
inline float mort_refshim_log(float x) { return mort_refshim_logf(x); }
inline double mort_refshim_log(double x) { return ::log(x); }

#define sinf(x) mort_refshim_sinf(x)
#define cosf(x) mort_refshim_cosf(x)
#define acosf(x) mort_refshim_acosf(x)
#define atan2f(y, x) mort_refshim_atan2f(y, x)
#define logf(x) mort_refshim_logf(x)
#define sin(x) mort_refshim_sin(x)
#define cos(x) mort_refshim_cos(x)
#define acos(x) mort_refshim_acos(x)
#define atan2(y, x) mort_refshim_atan2(y, x)
#define log(x) mort_refshim_log(x)

/* ---- MSVC's rand(): x = x * 214013 + 2531011, bits 16..30 of x ---- */
inline unsigned int &mort_refshim_rand_state() {
    static unsigned int s = 1u;
    return s;
}
inline void mort_refshim_srand(unsigned int seed) { mort_refshim_rand_state() = seed; }
inline int mort_refshim_rand() {
    unsigned int &s = mort_refshim_rand_state();
    s = s * 214013u + 2531011u;
    return int((s >> 16) & 0x7fffu);
}
#undef RAND_MAX
#define RAND_MAX 0x7fff
#define rand() mort_refshim_rand()
#define srand(s) mort_refshim_srand(s)

/* the reference's error-check macro comes from a header of its window layer */
#ifndef HANDLE_ERROR
#define HANDLE_ERROR(e) ((void)(e))
#endif

#endif /* MORT_REFSHIM_CUDA_RUNTIME_H */
