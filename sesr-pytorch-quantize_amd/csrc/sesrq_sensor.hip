// libsesrq_sensor.so: Bayer raw frames as sensors deliver them into the 3-channel nets (include/sesrq_sensor.h): four CFA orders, a
// black pedestal, white levels up to 16 bits, 16-bit containers or MIPI RAW10 / RAW12.  A library of its own: it links nothing of the
// other libraries and registers nothing in their instance tables.
//
// q0 and the fp32 frame are functions of d = clamp(code, black, white) - black and the Bayer phase only.  The fp32 frame is one
// correctly rounded division per pixel.  q0 is a map built on the host with the exact arithmetic of sesrq_forward's input quantiser
// (-ffp-contract=off): up to 4096 levels the table itself, staged in LDS once per workgroup as libsesrq_raw.so stages its table; for
// deeper sensors the table's steps: q0 is monotone in d and spans at most 255 codes, so the sorted d at which it steps
// up (a d repeated where it steps by more than one) fit 1 KiB, and q0(d) = q0(0) + #{steps <= d} is 8 LDS probes, uniform in their
// first levels.  The search compares integers the host derived from the table, so it returns the table's byte by construction.
//
// Kernel: a pure stream, 1.25 / 1.5 / 2 B/px read and 3 B/px written (+ 12 B/px for the fp32 frame).  Persistent grid-stride loop over
// row segments: 16 pixels of a packed row, a whole number of pack groups and of dwords (20 B of RAW10, 24 B of RAW12); 8 pixels of a
// U16 row, one 16-byte load as in libsesrq_raw.so (16-pixel segments halve the workgroups of a launch: 127 on 256 compute units at
// 540p).  A lane decodes its segment into codes in registers -- from 4-byte
// (packed) or 16-byte (U16) loads where the row's address allows, else byte by byte -- maps them, and writes one segment of q0 (and of
// fp32) per plane with 8- / 16-byte stores, or per pixel where W or the output addresses do not allow that.  The load and the store
// choice are independent of each other and of the map.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "sesrq_sensor.h"
#include "sesrq_side.h"

namespace sesrq_sensork {

constexpr int THREADS = 256;
constexpr int BLOCKS_PER_CU = 8;              // 256-thread blocks: a full CU (32 waves)
constexpr int TABLE_MAX = 4096;               // levels up to which the q0 map is the table
constexpr int MAP_BYTES = 4096;               // the device map: TABLE_MAX bytes of q0, or STEPS uint32 step positions and padding
constexpr int STEPS = 256;                    // 255 steps at most, padded with NO_STEP
constexpr uint32_t NO_STEP = 0xffffffffu;
enum { OUT_Q = 1, OUT_F = 2 };
enum { MAP_TABLE, MAP_STEPS };
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

// pixels per lane and segment, and the bytes that hold them
template <int PACK>
constexpr int seg_px() { return PACK == SESRQ_PACK_U16 ? 8 : 16; }
template <int PACK>
constexpr int seg_bytes() { return PACK == SESRQ_PACK_RAW10 ? 20 : PACK == SESRQ_PACK_RAW12 ? 24 : 16; }

// a whole segment from an address the wide loads can take (U16: 16-byte aligned, packed: 4-byte aligned)
template <int PACK>
__device__ inline void load_wide(const uint8_t *p, unsigned (&v)[seg_px<PACK>()]) {
    constexpr int SEG = seg_px<PACK>(), WORDS = seg_bytes<PACK>() / 4;
    unsigned w[WORDS];
    if constexpr (PACK == SESRQ_PACK_U16) {
        const uint4 a = *reinterpret_cast<const uint4 *>(p);
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
#pragma unroll
        for (int k = 0; k < SEG; ++k) v[k] = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
    } else {
#pragma unroll
        for (int i = 0; i < WORDS; ++i) w[i] = reinterpret_cast<const unsigned *>(p)[i];
        auto byte = [&](int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; };
        if constexpr (PACK == SESRQ_PACK_RAW10) {
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
    if constexpr (PACK == SESRQ_PACK_U16) {
        return (unsigned)row[2 * (size_t)x] | ((unsigned)row[2 * (size_t)x + 1] << 8);
    } else if constexpr (PACK == SESRQ_PACK_RAW10) {
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

template <int OUT, int MAP, int PACK>
__global__ __launch_bounds__(THREADS) void sensor_unpack(UnpackArgs a) {
    constexpr int SEG = seg_px<PACK>();
    __shared__ uint4 s_map4[THREADS];
    s_map4[threadIdx.x] = reinterpret_cast<const uint4 *>(a.map)[threadIdx.x];
    __syncthreads();
    const void *map = s_map4;
    const int t0 = a.t0;
    const unsigned z4 = (unsigned)(uint8_t)t0 * 0x01010101u;
    const int H = a.H, W = a.W;
    const unsigned black = a.black, white = a.white;
    const size_t plane = (size_t)H * W;
    for (int i = blockIdx.x * THREADS + threadIdx.x; i < a.items; i += gridDim.x * THREADS) {
        const int row = i / a.segs, seg = i - row * a.segs;
        const int n = row / H, y = row - n * H, x0 = seg * SEG;
        const int npx = min(SEG, W - x0);
        const int ph = a.sites >> (4 * (y & 1));
        const int ce = ph & 3, co = (ph >> 2) & 3;            // site channel of the even / the odd columns of this row
        const uint8_t *rowp = a.raw + (size_t)row * a.stride;
        const size_t base = ((size_t)n * 3 * H + y) * W + x0;  // plane (n, c, y) starts at base + c * plane

        unsigned d[SEG];
        if (a.in_vec && npx == SEG) {
            load_wide<PACK>(rowp + (size_t)seg * seg_bytes<PACK>(), d);
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k) d[k] = k < npx ? load_px<PACK>(rowp, x0 + k) : 0u;
        }
#pragma unroll
        for (int k = 0; k < SEG; ++k) d[k] = min(max(d[k], black), white) - black;

        if (a.out_vec) {             // W % SEG == 0: every segment is whole
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
                for (int k = 0; k < SEG; ++k) f[k] = __fdiv_rn((float)d[k], a.range);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float4 *dst = reinterpret_cast<float4 *>(a.spread + base + c * plane);
#pragma unroll
                    for (int j = 0; j < SEG / 4; ++j)
                        dst[j] = c == ce ? make_float4(f[4 * j], 0.f, f[4 * j + 2], 0.f)
                                 : c == co ? make_float4(0.f, f[4 * j + 1], 0.f, f[4 * j + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k) {
                const int cs = (k & 1) ? co : ce;
                if ((OUT & OUT_Q) && k < npx) {
                    const int8_t q = (int8_t)q_of<MAP>(map, d[k], t0);
#pragma unroll
                    for (int c = 0; c < 3; ++c) a.q0[base + c * plane + k] = c == cs ? q : (int8_t)t0;
                }
                if ((OUT & OUT_F) && k < npx) {
                    const float f = __fdiv_rn((float)d[k], a.range);
#pragma unroll
                    for (int c = 0; c < 3; ++c) a.spread[base + c * plane + k] = c == cs ? f : 0.f;
                }
            }
        }
    }
}

}  // namespace sesrq_sensork

using namespace sesrq_sensork;

struct sesrq_sensor_ctx_s {
    DeviceTable t;     // MAP_BYTES of the q0 map
    sesrq_sensor_format fmt;
    int map, t0;
};

// one instantiation per (packing, map, output set); a packed format has at most 4096 levels, so it never takes the steps
enum { F_U16_TABLE, F_U16_STEPS, F_RAW10, F_RAW12, F_COUNT };
enum { K_COUNT = F_COUNT * 3 };
static const char *const kNames[K_COUNT] = {
    "sensor_unpack<u16,table,q0>",   "sensor_unpack<u16,table,spread>",   "sensor_unpack<u16,table,q0+spread>",
    "sensor_unpack<u16,steps,q0>",   "sensor_unpack<u16,steps,spread>",   "sensor_unpack<u16,steps,q0+spread>",
    "sensor_unpack<raw10,table,q0>", "sensor_unpack<raw10,table,spread>", "sensor_unpack<raw10,table,q0+spread>",
    "sensor_unpack<raw12,table,q0>", "sensor_unpack<raw12,table,spread>", "sensor_unpack<raw12,table,q0+spread>"};
static Counters<K_COUNT> g_count{kNames};

static const int kSites[4] = {0 | 1 << 2 | 1 << 4 | 2 << 6, 1 | 0 << 2 | 2 << 4 | 1 << 6, 1 | 2 << 2 | 0 << 4 | 1 << 6,
                              2 | 1 << 2 | 1 << 4 | 0 << 6};

static int check_format(const char *who, const sesrq_sensor_format *f) {
    if (!f) return fail("%s: format is NULL", who);
    if (f->cfa < SESRQ_CFA_RGGB || f->cfa > SESRQ_CFA_BGGR) return fail("%s: cfa %d is not a Bayer order (0 .. 3)", who, f->cfa);
    if (f->packing < SESRQ_PACK_U16 || f->packing > SESRQ_PACK_RAW12) return fail("%s: packing %d (0 u16, 1 raw10, 2 raw12)", who, f->packing);
    if (f->black < 0 || f->black >= f->white || f->white > 65535)
        return fail("%s: levels need 0 <= black < white <= 65535, got black %d, white %d", who, f->black, f->white);
    const int top = f->packing == SESRQ_PACK_RAW10 ? 1023 : f->packing == SESRQ_PACK_RAW12 ? 4095 : 65535;
    if (f->white > top) return fail("%s: white %d is above the packing's range (%d)", who, f->white, top);
    return 0;
}

static size_t row_bytes(const char *who, const sesrq_sensor_format *f, int W) {
    if (W < 1) return fail("%s: W = %d", who, W), 0;
    const int group = f->packing == SESRQ_PACK_RAW10 ? 4 : f->packing == SESRQ_PACK_RAW12 ? 2 : 1;
    if (W % group) return fail("%s: W = %d is not a multiple of the %d pixels of a pack group", who, W, group), 0;
    return f->packing == SESRQ_PACK_RAW10 ? (size_t)W / 4 * 5 : f->packing == SESRQ_PACK_RAW12 ? (size_t)W / 2 * 3 : (size_t)W * 2;
}

extern "C" size_t sesrq_sensor_row_bytes(const sesrq_sensor_format *fmt, int W) {
    g_err[0] = 0;
    if (check_format("sesrq_sensor_row_bytes", fmt)) return 0;
    return row_bytes("sesrq_sensor_row_bytes", fmt, W);
}

extern "C" int sesrq_sensor_table(const sesrq_sensor_format *fmt, float scale_in, int zero_in, int exact_div, int8_t *table, size_t entries) {
    g_err[0] = 0;
    if (!table) return fail("sesrq_sensor_table: table is NULL");
    if (check_format("sesrq_sensor_table", fmt)) return 1;
    if (check_domain("sesrq_sensor_table", scale_in, zero_in, exact_div)) return 1;
    const int D = fmt->white - fmt->black;
    if (entries != (size_t)D + 1) return fail("sesrq_sensor_table: %zu entries, the format has white - black + 1 = %d", entries, D + 1);
    const InQuant q = in_quant(scale_in, zero_in, exact_div);
    for (int d = 0; d <= D; ++d) {
        float x = (float)d / (float)D;                       // true IEEE quotient, as torch's CPU tensor / scalar
        x = fminf(fmaxf(x, 0.f), 1.f);
        table[d] = host_quant(x, q);
    }
    return 0;
}

extern "C" int sesrq_sensor_create(const sesrq_sensor_format *fmt, float scale_in, int zero_in, int exact_div, sesrq_sensor_ctx *out) {
    g_err[0] = 0;
    if (!out) return fail("sesrq_sensor_create: ctx is NULL");
    *out = nullptr;
    if (check_format("sesrq_sensor_create", fmt)) return 1;
    const int levels = fmt->white - fmt->black + 1;
    std::vector<int8_t> table(levels);
    if (sesrq_sensor_table(fmt, scale_in, zero_in, exact_div, table.data(), table.size())) return 1;
    alignas(16) uint8_t host[MAP_BYTES] = {};
    const int map = levels <= TABLE_MAX ? MAP_TABLE : MAP_STEPS;
    if (map == MAP_TABLE) {
        for (int d = 0; d < levels; ++d) host[d] = (uint8_t)table[d];
    } else {
        uint32_t *step = reinterpret_cast<uint32_t *>(host);
        int n = 0;
        for (int d = 1; d < levels; ++d) {
            if (table[d] < table[d - 1]) return fail("sesrq_sensor_create: the q0 table is not monotone at %d", d);
            for (int k = table[d - 1]; k < table[d]; ++k) step[n++] = (uint32_t)d;      // at most 255 in all: the table is int8
        }
        for (; n < STEPS; ++n) step[n] = NO_STEP;
    }
    auto *c = new sesrq_sensor_ctx_s();
    c->fmt = *fmt;
    c->map = map;
    c->t0 = table[0];
    const hipError_t e = table_create(c->t, host, MAP_BYTES);
    if (e != hipSuccess) {
        delete c;
        return fail("sesrq_sensor_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return 0;
}

extern "C" void sesrq_sensor_destroy(sesrq_sensor_ctx c) {
    if (!c) return;
    table_destroy(c->t);
    delete c;
}

template <int MAP, int PACK>
static void launch(int outs, int grid, hipStream_t st, const UnpackArgs &a) {
    if (outs == (OUT_Q | OUT_F))
        sensor_unpack<OUT_Q | OUT_F, MAP, PACK><<<grid, THREADS, 0, st>>>(a);
    else if (outs == OUT_Q)
        sensor_unpack<OUT_Q, MAP, PACK><<<grid, THREADS, 0, st>>>(a);
    else
        sensor_unpack<OUT_F, MAP, PACK><<<grid, THREADS, 0, st>>>(a);
}

extern "C" int sesrq_sensor_unpack(sesrq_sensor_ctx c, const void *raw, size_t row_stride_bytes, int8_t *q0, float *spread, int N, int H,
                                   int W, void *stream) {
    g_err[0] = 0;
    if (!c) return fail("sesrq_sensor_unpack: ctx is NULL");
    if (!raw) return fail("sesrq_sensor_unpack: raw is NULL");
    if (!q0 && !spread) return fail("sesrq_sensor_unpack: neither q0 nor spread requested");
    if (N < 1 || H < 1 || W < 1) return fail("sesrq_sensor_unpack: empty frame (N = %d, H = %d, W = %d)", N, H, W);
    const size_t need = row_bytes("sesrq_sensor_unpack", &c->fmt, W);
    if (!need) return 1;
    if (row_stride_bytes < need)
        return fail("sesrq_sensor_unpack: row_stride_bytes %zu is less than the %zu bytes of a row of %d pixels", row_stride_bytes, need, W);
    if (reinterpret_cast<uintptr_t>(spread) % 4) return fail("sesrq_sensor_unpack: spread is not 4-byte aligned");
    const int pack = c->fmt.packing;
    const int SEG = pack == SESRQ_PACK_U16 ? seg_px<SESRQ_PACK_U16>() : seg_px<SESRQ_PACK_RAW10>();
    static_assert(seg_px<SESRQ_PACK_RAW10>() == seg_px<SESRQ_PACK_RAW12>(), "one segment length for the packed formats");
    const long long segs = (W + SEG - 1) / SEG, items = (long long)N * H * segs;
    if (items > 0x7fffffffLL - (long long)THREADS * c->t.num_cu * BLOCKS_PER_CU)
        return fail("sesrq_sensor_unpack: frame of %d x %d x %d is too large", N, H, W);
    if (table_on_current("sesrq_sensor_unpack", c->t)) return 1;

    const uintptr_t in_align = pack == SESRQ_PACK_U16 ? 16 : 4;
    UnpackArgs a;
    a.raw = static_cast<const uint8_t *>(raw);
    a.map = c->t.ptr;
    a.q0 = q0;
    a.spread = spread;
    a.stride = row_stride_bytes;
    a.H = H;
    a.W = W;
    a.segs = (int)segs;
    a.items = (int)items;
    a.black = c->fmt.black;
    a.white = c->fmt.white;
    a.range = (float)(c->fmt.white - c->fmt.black);
    a.sites = kSites[c->fmt.cfa];
    a.t0 = c->t0;
    a.in_vec = reinterpret_cast<uintptr_t>(raw) % in_align == 0 && row_stride_bytes % in_align == 0;
    a.out_vec = W % SEG == 0 && reinterpret_cast<uintptr_t>(q0) % SEG == 0 && reinterpret_cast<uintptr_t>(spread) % 16 == 0;
    const int grid = grid_cap(items, THREADS, c->t.num_cu, BLOCKS_PER_CU);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int outs = (q0 ? OUT_Q : 0) | (spread ? OUT_F : 0);
    int family;
    if (pack == SESRQ_PACK_RAW10) {
        family = F_RAW10;
        launch<MAP_TABLE, SESRQ_PACK_RAW10>(outs, grid, st, a);
    } else if (pack == SESRQ_PACK_RAW12) {
        family = F_RAW12;
        launch<MAP_TABLE, SESRQ_PACK_RAW12>(outs, grid, st, a);
    } else if (c->map == MAP_TABLE) {
        family = F_U16_TABLE;
        launch<MAP_TABLE, SESRQ_PACK_U16>(outs, grid, st, a);
    } else {
        family = F_U16_STEPS;
        launch<MAP_STEPS, SESRQ_PACK_U16>(outs, grid, st, a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("sesrq_sensor_unpack: kernel launch: %s", hipGetErrorString(e));
    ++g_count.launches[family * 3 + outs - 1];
    return 0;
}

extern "C" int sesrq_sensor_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_sensor_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_sensor_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_sensor_last_error(void) { return g_err; }
