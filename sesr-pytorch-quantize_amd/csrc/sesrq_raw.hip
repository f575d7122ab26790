// libsesrq_raw.so: 12-bit RGGB Bayer raw frames into the 3-channel nets (include/sesrq_raw.h).  A library of its own: it links nothing
// of libsesrq.so and registers nothing in its instance table.
//
// The reference (self_dataset.py TestDataset.__getitem__) spreads a uint16 raw frame into a sparse 3-channel RGGB mosaic, divides by
// 4095 in fp32 and clamps to [0, 1]; its integer path then quantises that frame into q0.  Both steps are a function of the 12-bit code
// and the Bayer phase only, so q0 is one lookup in a 4096-entry table built on the host (the exact arithmetic of sesrq_forward's input
// quantiser, -ffp-contract=off), and the fp32 frame is one correctly rounded division per pixel.
//
// Kernel: the Bayer unpack body the sensor library shares (sesrq_bayer_unpack.h) at the reference's format, fixed at compile time: a
// pure stream, 2 B/px read and 3 B/px written (+ 12 B/px for the fp32 frame).  Persistent grid-stride loop over row segments of 8
// pixels; the table is staged in LDS once per workgroup.  A lane loads its segment with one 16-byte load, clamps each code to 4095,
// gathers 8 table bytes from LDS and writes 8 bytes of q0 (and 32 bytes of fp32) per plane.  Rows whose start is not 16-byte aligned
// (W % 8 != 0, or unaligned buffers) take the per-pixel path of the same kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sesrq_bayer_unpack.h"
#include "sesrq_raw.h"
#include "sesrq_side.h"

namespace sesrq_rawk {

using namespace sesrq_bayer;
constexpr int SEG = seg_px<PACK_U16>();       // pixels per lane and segment
constexpr int CODE_MAX = SESRQ_RAW_CODES - 1;
static_assert(SESRQ_RAW_CODES == MAP_BYTES, "the table is the body's MAP_TABLE layout");

template <int OUT>
__global__ __launch_bounds__(THREADS) void raw_unpack(UnpackArgs a) {
    unpack<OUT, MAP_TABLE, PACK_U16, true>(a);
}

}  // namespace sesrq_rawk

using namespace sesrq_rawk;

struct sesrq_raw_ctx_s {
    DeviceTable t;     // SESRQ_RAW_CODES bytes of q0
    int t0;            // q0 of code 0
};

enum { K_Q = 0, K_F, K_QF, K_COUNT };
static const char *const kNames[K_COUNT] = {"raw_unpack<q0>", "raw_unpack<spread>", "raw_unpack<q0,spread>"};
static Counters<K_COUNT> g_count{kNames};

extern "C" int sesrq_raw_table(float scale_in, int zero_in, int exact_div, int8_t table[SESRQ_RAW_CODES]) {
    g_err[0] = 0;
    if (!table) return fail("sesrq_raw_table: table is NULL");
    if (check_domain("sesrq_raw_table", scale_in, zero_in, exact_div)) return 1;
    level_table(CODE_MAX, in_quant(scale_in, zero_in, exact_div), table);
    return 0;
}

extern "C" int sesrq_raw_create(float scale_in, int zero_in, int exact_div, sesrq_raw_ctx *out) {
    g_err[0] = 0;
    if (!out) return fail("sesrq_raw_create: ctx is NULL");
    *out = nullptr;
    int8_t host[SESRQ_RAW_CODES];
    if (sesrq_raw_table(scale_in, zero_in, exact_div, host)) return 1;
    auto *c = new sesrq_raw_ctx_s();
    c->t0 = host[0];
    return ctx_publish("sesrq_raw_create", c, host, SESRQ_RAW_CODES, out);
}

extern "C" void sesrq_raw_destroy(sesrq_raw_ctx c) { ctx_destroy(c); }

extern "C" int sesrq_raw_unpack(sesrq_raw_ctx c, const uint16_t *raw, int8_t *q0, float *spread, int N, int H, int W, void *stream) {
    g_err[0] = 0;
    if (check_unpack("sesrq_raw_unpack", c, raw, q0, spread, N, H, W)) return 1;
    UnpackArgs a = {};     // the format fields stay unread: the body has them as constants
    if (segment_items("sesrq_raw_unpack", N, H, W, SEG, (long long)THREADS * c->t.num_cu * BLOCKS_PER_CU, &a.segs, &a.items)) return 1;
    if (table_on_current("sesrq_raw_unpack", c->t)) return 1;

    a.raw = reinterpret_cast<const uint8_t *>(raw);
    a.map = c->t.ptr;
    a.q0 = q0;
    a.spread = spread;
    a.H = H;
    a.W = W;
    a.t0 = c->t0;
    // one predicate for the load and the store choice ("Caller buffers")
    a.in_vec = a.out_vec = W % SEG == 0 && reinterpret_cast<uintptr_t>(raw) % 16 == 0 && reinterpret_cast<uintptr_t>(q0) % 8 == 0 &&
                           reinterpret_cast<uintptr_t>(spread) % 16 == 0;
    const int grid = grid_cap(a.items, THREADS, c->t.num_cu, BLOCKS_PER_CU);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int k;
    if (q0 && spread) {
        k = K_QF;
        raw_unpack<OUT_Q | OUT_F><<<grid, THREADS, 0, st>>>(a);
    } else if (q0) {
        k = K_Q;
        raw_unpack<OUT_Q><<<grid, THREADS, 0, st>>>(a);
    } else {
        k = K_F;
        raw_unpack<OUT_F><<<grid, THREADS, 0, st>>>(a);
    }
    return launched("sesrq_raw_unpack", g_count, k);
}

extern "C" int sesrq_raw_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_raw_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_raw_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_raw_last_error(void) { return g_err; }
