// The Bayer unpack both raw libraries run (csrc/sesrq_raw.hip, csrc/sesrq_sensor.hip): device code and its argument struct only.  Each
// library compiles its own copy into __global__ wrappers of its own names (they share no symbol), with -ffp-contract=off.
//
// The body is a pure stream, 1.25 / 1.5 / 2 B/px read and 3 B/px written (+ 12 B/px for the fp32 frame): the q0 map is staged in LDS
// once per workgroup, then a persistent grid-stride loop walks row segments -- 16 pixels of a packed row, a whole number of pack groups
// and of dwords (20 B of RAW10, 24 B of RAW12); 8 pixels of a U16 row, one 16-byte load (16-pixel segments halve the workgroups of a
// launch: 127 on 256 compute units at 540p).  A lane decodes its segment into codes in registers -- from 4-byte (packed)
// or 16-byte (U16) loads where the row's address allows, else byte by byte -- maps them, and writes one segment of q0 (and of fp32)
// per plane with 8- / 16-byte stores, or per pixel where W or the output addresses do not allow that.
//
// REF fixes the reference's dataset format at compile time (libsesrq_raw.so): black 0, white 4095, range 4095.0f, the RGGB site
// channels, rows 2 W bytes apart, and one predicate (in_vec) for the load and the store choice -- sesrq_raw_unpack takes the wide path
// only where both hold, so the two mixed combinations are not compiled.  Without REF all of these are arguments, and the load choice
// (address, stride) and the store choice (W, output addresses) are independent of each other and of the map.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sesrq_bayer {

constexpr int THREADS = 256;
constexpr int BLOCKS_PER_CU = 8;              // 256-thread blocks: a full CU (32 waves)
constexpr int MAP_BYTES = 4096;               // the device map: 4096 bytes of q0, or STEPS uint32 step positions and padding
constexpr int STEPS = 256;                    // 255 steps at most, padded with NO_STEP
constexpr uint32_t NO_STEP = 0xffffffffu;
enum { OUT_Q = 1, OUT_F = 2 };
enum { MAP_TABLE, MAP_STEPS };
enum { PACK_U16, PACK_RAW10, PACK_RAW12 };    // = SESRQ_PACK_* of include/sesrq_sensor.h
static_assert(MAP_BYTES == THREADS * 16, "one 16-byte load per thread stages the map");

struct UnpackArgs {
    const uint8_t *raw;
    const void *map;       // device, MAP_BYTES
    int8_t *q0;
    float *spread;
    size_t stride;         // bytes between rows
    int H, W, segs, items;
    int black, white;
    float range;           // fl32(white - black), exact
    int sites;             // 2 bits per parity (py * 2 + px): its site channel
    int t0;                // q0 of x = 0.0f: the map's first byte
    int in_vec, out_vec;
};

// 2 bits per parity of each CFA order (SESRQ_CFA_* of include/sesrq_sensor.h), as UnpackArgs::sites takes them
constexpr int SITES[4] = {0 | 1 << 2 | 1 << 4 | 2 << 6, 1 | 0 << 2 | 2 << 4 | 1 << 6, 1 | 2 << 2 | 0 << 4 | 1 << 6,
                          2 | 1 << 2 | 1 << 4 | 0 << 6};

// pixels per lane and segment, and the bytes that hold them
template <int PACK>
constexpr int seg_px() { return PACK == PACK_U16 ? 8 : 16; }
template <int PACK>
constexpr int seg_bytes() { return PACK == PACK_RAW10 ? 20 : PACK == PACK_RAW12 ? 24 : 16; }

// a whole segment from an address the wide loads can take (U16: 16-byte aligned, packed: 4-byte aligned)
template <int PACK>
__device__ inline void load_wide(const uint8_t *p, unsigned (&v)[seg_px<PACK>()]) {
    constexpr int SEG = seg_px<PACK>(), WORDS = seg_bytes<PACK>() / 4;
    unsigned w[WORDS];
    if constexpr (PACK == PACK_U16) {
        const uint4 a = *reinterpret_cast<const uint4 *>(p);
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
#pragma unroll
        for (int k = 0; k < SEG; ++k) v[k] = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
    } else {
#pragma unroll
        for (int i = 0; i < WORDS; ++i) w[i] = reinterpret_cast<const unsigned *>(p)[i];
        auto byte = [&](int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; };
        if constexpr (PACK == PACK_RAW10) {
#pragma unroll
            for (int g = 0; g < SEG / 4; ++g) {
                const unsigned lo = byte(5 * g + 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[4 * g + k] = (byte(5 * g + k) << 2) | ((lo >> (2 * k)) & 3u);
            }
        } else {
#pragma unroll
            for (int g = 0; g < SEG / 2; ++g) {
                const unsigned lo = byte(3 * g + 2);
                v[2 * g] = (byte(3 * g) << 4) | (lo & 0xfu);
                v[2 * g + 1] = (byte(3 * g + 1) << 4) | (lo >> 4);
            }
        }
    }
}

// pixel x of the row at `row`, byte by byte: any address, and no byte behind the row's last pack group
template <int PACK>
__device__ inline unsigned load_px(const uint8_t *row, int x) {
    if constexpr (PACK == PACK_U16) {
        return (unsigned)row[2 * (size_t)x] | ((unsigned)row[2 * (size_t)x + 1] << 8);
    } else if constexpr (PACK == PACK_RAW10) {
        const uint8_t *g = row + (size_t)(x >> 2) * 5;
        return ((unsigned)g[x & 3] << 2) | (((unsigned)g[4] >> (2 * (x & 3))) & 3u);
    } else {
        const uint8_t *g = row + (size_t)(x >> 1) * 3;
        return (x & 1) ? ((unsigned)g[1] << 4) | ((unsigned)g[2] >> 4) : ((unsigned)g[0] << 4) | ((unsigned)g[2] & 0xfu);
    }
}

template <int MAP>
__device__ inline unsigned q_of(const void *lds, unsigned d, int t0) {
    if constexpr (MAP == MAP_TABLE) {
        return (unsigned)static_cast<const uint8_t *>(lds)[d];
    } else {
        // #{steps <= d} in the sorted, NO_STEP-padded list: entries 0 .. STEPS - 2 are probed, so the count is at most STEPS - 1
        const uint32_t *step = static_cast<const uint32_t *>(lds);
        int n = 0;
#pragma unroll
        for (int h = STEPS / 2; h >= 1; h >>= 1) n += step[n + h - 1] <= d ? h : 0;
        return (unsigned)(t0 + n) & 0xffu;
    }
}

// The whole kernel: a __global__ wrapper of THREADS threads calls this and nothing else.
template <int OUT, int MAP, int PACK, bool REF>
__device__ __forceinline__ void unpack(const UnpackArgs &a) {
    constexpr int SEG = seg_px<PACK>();
    static_assert(!REF || (MAP == MAP_TABLE && PACK == PACK_U16), "the reference's format is 4096 levels in uint16");
    __shared__ uint4 s_map4[THREADS];
    s_map4[threadIdx.x] = reinterpret_cast<const uint4 *>(a.map)[threadIdx.x];
    __syncthreads();
    const void *map = s_map4;
    const int t0 = a.t0;
    const unsigned z4 = (unsigned)(uint8_t)t0 * 0x01010101u;
    const int H = a.H, W = a.W;
    const unsigned black = REF ? 0u : (unsigned)a.black, white = REF ? 4095u : (unsigned)a.white;
    const float range = REF ? 4095.f : a.range;
    const size_t plane = (size_t)H * W;
    for (int i = blockIdx.x * THREADS + threadIdx.x; i < a.items; i += gridDim.x * THREADS) {
        const int row = i / a.segs, seg = i - row * a.segs;
        const int n = row / H, y = row - n * H, x0 = seg * SEG;
        const int npx = min(SEG, W - x0);
        // site channel of the even / the odd columns of this row; RGGB: R (py 0) / G (py 1) and G / B
        const int ph = a.sites >> (4 * (y & 1));
        const int ce = REF ? y & 1 : ph & 3, co = REF ? ce + 1 : (ph >> 2) & 3;
        const uint8_t *rowp = a.raw + (REF ? 2 * ((size_t)row * W) : (size_t)row * a.stride);
        const size_t base = ((size_t)n * 3 * H + y) * W + x0;  // plane (n, c, y) starts at base + c * plane

        unsigned d[SEG];
        auto load = [&](bool wide) {
            if (wide) {
                load_wide<PACK>(rowp + (size_t)seg * seg_bytes<PACK>(), d);
            } else {
#pragma unroll
                for (int k = 0; k < SEG; ++k)      // REF: the rows are uint16_t's
                    d[k] = k >= npx ? 0u : REF ? reinterpret_cast<const uint16_t *>(rowp)[x0 + k] : load_px<PACK>(rowp, x0 + k);
            }
#pragma unroll
            for (int k = 0; k < SEG; ++k) d[k] = min(max(d[k], black), white) - black;
        };
        auto store_wide = [&]() {    // W % SEG == 0: every segment is whole
            if (OUT & OUT_Q) {
                // E: the even columns' q0, O: the odd columns', q0(0) elsewhere
                unsigned e[SEG / 4], o[SEG / 4];
#pragma unroll
                for (int j = 0; j < SEG / 4; ++j) {
                    e[j] = (z4 & 0xff00ff00u) | q_of<MAP>(map, d[4 * j], t0) | (q_of<MAP>(map, d[4 * j + 2], t0) << 16);
                    o[j] = (z4 & 0x00ff00ffu) | (q_of<MAP>(map, d[4 * j + 1], t0) << 8) | (q_of<MAP>(map, d[4 * j + 3], t0) << 24);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const unsigned *src = c == ce ? e : o;
                    const bool site = c == ce || c == co;
                    if constexpr (SEG == 16)
                        *reinterpret_cast<uint4 *>(a.q0 + base + c * plane) =
                            site ? make_uint4(src[0], src[1], src[2], src[3]) : make_uint4(z4, z4, z4, z4);
                    else
                        *reinterpret_cast<uint2 *>(a.q0 + base + c * plane) = site ? make_uint2(src[0], src[1]) : make_uint2(z4, z4);
                }
            }
            if (OUT & OUT_F) {
                float f[SEG];
#pragma unroll
                for (int k = 0; k < SEG; ++k) f[k] = __fdiv_rn((float)d[k], range);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float4 *dst = reinterpret_cast<float4 *>(a.spread + base + c * plane);
#pragma unroll
                    for (int j = 0; j < SEG / 4; ++j)
                        dst[j] = c == ce ? make_float4(f[4 * j], 0.f, f[4 * j + 2], 0.f)
                                 : c == co ? make_float4(0.f, f[4 * j + 1], 0.f, f[4 * j + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        };
        auto store_px = [&]() {
#pragma unroll
            for (int k = 0; k < SEG; ++k) {
                const int cs = (k & 1) ? co : ce;
                if ((OUT & OUT_Q) && k < npx) {
                    const int8_t q = (int8_t)q_of<MAP>(map, d[k], t0);
#pragma unroll
                    for (int c = 0; c < 3; ++c) a.q0[base + c * plane + k] = c == cs ? q : (int8_t)t0;
                }
                if ((OUT & OUT_F) && k < npx) {
                    const float f = __fdiv_rn((float)d[k], range);
#pragma unroll
                    for (int c = 0; c < 3; ++c) a.spread[base + c * plane + k] = c == cs ? f : 0.f;
                }
            }
        };
        if constexpr (REF) {
            if (a.in_vec) {
                load(true);
                store_wide();
            } else {
                load(false);
                store_px();
            }
        } else {
            load(a.in_vec && npx == SEG);
            if (a.out_vec)
                store_wide();
            else
                store_px();
        }
    }
}

}  // namespace sesrq_bayer
