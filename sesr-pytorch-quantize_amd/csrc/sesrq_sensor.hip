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
// Kernel: the Bayer unpack body libsesrq_raw.so shares (sesrq_bayer_unpack.h, which describes the stream), with the format in its
// arguments and one instantiation per (packing, map, output set).  The load and the store choice are independent of each other and of
// the map.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "sesrq_bayer_unpack.h"
#include "sesrq_sensor.h"
#include "sesrq_side.h"

namespace sesrq_sensork {

using namespace sesrq_bayer;
constexpr int TABLE_MAX = MAP_BYTES;          // levels up to which the q0 map is the table
static_assert(PACK_U16 == SESRQ_PACK_U16 && PACK_RAW10 == SESRQ_PACK_RAW10 && PACK_RAW12 == SESRQ_PACK_RAW12, "the body's packings are the header's");

template <int OUT, int MAP, int PACK>
__global__ __launch_bounds__(THREADS) void sensor_unpack(UnpackArgs a) {
    unpack<OUT, MAP, PACK, false>(a);
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
    level_table(D, in_quant(scale_in, zero_in, exact_div), table);
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
    return ctx_publish("sesrq_sensor_create", c, host, MAP_BYTES, out);
}

extern "C" void sesrq_sensor_destroy(sesrq_sensor_ctx c) { ctx_destroy(c); }

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
    if (check_unpack("sesrq_sensor_unpack", c, raw, q0, spread, N, H, W)) return 1;
    const size_t need = row_bytes("sesrq_sensor_unpack", &c->fmt, W);
    if (!need) return 1;
    if (row_stride_bytes < need)
        return fail("sesrq_sensor_unpack: row_stride_bytes %zu is less than the %zu bytes of a row of %d pixels", row_stride_bytes, need, W);
    if (reinterpret_cast<uintptr_t>(spread) % 4) return fail("sesrq_sensor_unpack: spread is not 4-byte aligned");
    const int pack = c->fmt.packing;
    const int SEG = pack == SESRQ_PACK_U16 ? seg_px<PACK_U16>() : seg_px<PACK_RAW10>();
    static_assert(seg_px<PACK_RAW10>() == seg_px<PACK_RAW12>(), "one segment length for the packed formats");
    UnpackArgs a;
    if (segment_items("sesrq_sensor_unpack", N, H, W, SEG, (long long)THREADS * c->t.num_cu * BLOCKS_PER_CU, &a.segs, &a.items)) return 1;
    if (table_on_current("sesrq_sensor_unpack", c->t)) return 1;

    const uintptr_t in_align = pack == SESRQ_PACK_U16 ? 16 : 4;
    a.raw = static_cast<const uint8_t *>(raw);
    a.map = c->t.ptr;
    a.q0 = q0;
    a.spread = spread;
    a.stride = row_stride_bytes;
    a.H = H;
    a.W = W;
    a.black = c->fmt.black;
    a.white = c->fmt.white;
    a.range = (float)(c->fmt.white - c->fmt.black);
    a.sites = SITES[c->fmt.cfa];
    a.t0 = c->t0;
    a.in_vec = reinterpret_cast<uintptr_t>(raw) % in_align == 0 && row_stride_bytes % in_align == 0;
    a.out_vec = W % SEG == 0 && reinterpret_cast<uintptr_t>(q0) % SEG == 0 && reinterpret_cast<uintptr_t>(spread) % 16 == 0;
    const int grid = grid_cap(a.items, THREADS, c->t.num_cu, BLOCKS_PER_CU);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int outs = (q0 ? OUT_Q : 0) | (spread ? OUT_F : 0);
    int family;
    if (pack == SESRQ_PACK_RAW10) {
        family = F_RAW10;
        launch<MAP_TABLE, PACK_RAW10>(outs, grid, st, a);
    } else if (pack == SESRQ_PACK_RAW12) {
        family = F_RAW12;
        launch<MAP_TABLE, PACK_RAW12>(outs, grid, st, a);
    } else if (c->map == MAP_TABLE) {
        family = F_U16_TABLE;
        launch<MAP_TABLE, PACK_U16>(outs, grid, st, a);
    } else {
        family = F_U16_STEPS;
        launch<MAP_STEPS, PACK_U16>(outs, grid, st, a);
    }
    return launched("sesrq_sensor_unpack", g_count, family * 3 + outs - 1);
}

extern "C" int sesrq_sensor_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_sensor_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_sensor_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_sensor_last_error(void) { return g_err; }
