// The decode of 8-bit image bytes into the super-resolution nets' input (include/sesrq_image.h, which fixes the arithmetic): the tables
// of a context, how the host builds them, and the per-pixel device body -- the float64 luma of the Y form, the table lookup of the RGB
// form, the input quantiser.  libsesrq_image.so (image_decode: bytes from memory) and libsesrq_downscale.so (bytes from its own bicubic
// pass) both instantiate it, so the arithmetic stands once.  Each library stays a library of its own; everything here has internal
// linkage.  Include after sesrq_side.h (InQuant, host_quant).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_image.h"

namespace sesrq_imgdec {

constexpr int CODES = SESRQ_IMAGE_CODES;

// one device allocation per context
struct Tables {
    double y[3][CODES];   // 65.481 d(v), 128.553 d(v), 24.966 d(v): the Y form's three products, each rounded once in float64
    float x[CODES];       // RGB form: clip(fl32(d(v)), 0, 1)
    int8_t q[CODES];      // RGB form: q0 of x[v]
};
constexpr int Y_WORDS = sizeof(double) * 3 * CODES / 16;                    // 384
constexpr int RGB_WORDS = (sizeof(float) + 1) * CODES / 16;                  // 80
static_assert(sizeof(Tables) == 16 * (Y_WORDS + RGB_WORDS), "tables are whole 16-byte words");

// the 16-byte words a form reads: the Y form the three product tables, the RGB form x and q
template <int FORM>
constexpr int table_words() { return FORM == SESRQ_IMAGE_Y ? Y_WORDS : RGB_WORDS; }

// quantiser: x / s0 (recip 0) or x * r0 (recip 1), + z0
struct Quant {
    float s0, r0, z0;
    int recip;
};

__device__ inline int8_t quant(float x, const Quant &a) {
    const float t = a.recip ? __fmul_rn(x, a.r0) : __fdiv_rn(x, a.s0);
    return (int8_t)fminf(fmaxf(rintf(__fadd_rn(t, a.z0)), -128.f), 127.f);
}

// the Y form of one pixel from its three bytes (R, G, B)
__device__ inline float luma(const double (*ty)[CODES], unsigned r, unsigned g, unsigned b) {
    double s = __dadd_rn(ty[0][r], ty[1][g]);
    s = __dadd_rn(s, ty[2][b]);
    s = __dadd_rn(s, 16.0);
    const double y = __ddiv_rn(s, 255.0);                 // a true quotient: no reciprocal multiply
    return (float)fmin(fmax(y, 0.0), 1.0);
}

// a form's tables from the context's allocation into LDS (s_tab: table_words<FORM>() 16-byte words); the caller synchronises
template <int FORM, int THREADS>
__device__ inline void stage_tables(uint4 *s_tab, const Tables *tab) {
    const uint4 *g4 = reinterpret_cast<const uint4 *>(FORM == SESRQ_IMAGE_Y ? (const void *)tab->y : (const void *)tab->x);
    for (int k = threadIdx.x; k < table_words<FORM>(); k += THREADS) s_tab[k] = g4[k];
}

// the staged tables as the forms read them
__device__ inline const double (*table_y(const uint4 *s_tab))[CODES] { return reinterpret_cast<const double(*)[CODES]>(s_tab); }
__device__ inline const float *table_x(const uint4 *s_tab) { return reinterpret_cast<const float *>(s_tab); }
__device__ inline const int8_t *table_q(const uint4 *s_tab) { return reinterpret_cast<const int8_t *>(table_x(s_tab) + CODES); }

static inline Quant quant_of(const InQuant &q) { return {q.s0, q.r0, q.z0, q.recip}; }

static inline void build(const InQuant &q, Tables &t) {
    for (int v = 0; v < CODES; ++v) {
        const volatile double d = (double)v / 255.0;      // d(v), correctly rounded
        t.y[0][v] = 65.481 * d;
        t.y[1][v] = 128.553 * d;
        t.y[2][v] = 24.966 * d;
        const float x = fminf(fmaxf((float)d, 0.f), 1.f);
        t.x[v] = x;
        t.q[v] = host_quant(x, q);
    }
}

}  // namespace sesrq_imgdec
