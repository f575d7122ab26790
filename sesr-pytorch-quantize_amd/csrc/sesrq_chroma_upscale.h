// What the bicubic chroma upscale of the colour and of the video export have in common (csrc/sesrq_colour.hip, csrc/sesrq_video.hip):
// device code only.  Each library compiles its own copy into its own __global__ kernels (they share no symbol).
//
// Shared: the Keys a = -1/2 weight table x 1024 (include/sesrq_colour.h fixes it, include/sesrq_video.h takes it over), the offset
// of a phase's first tap, the select of a lane's own weights and the half-word extract; the rule that pads the rows between the two
// passes.
//
// Each library keeps what is its own: where the staged Q6 samples come from, which lane takes which output row and run, every
// address, what becomes of the upscaled samples and of the luma, the walk from blockIdx.x to a tile and a frame -- and three bodies
// that are the same text in both kernels: a lane's luma load (fp32 / int8 x 16-byte / per element, requested before the tile is
// staged), the horizontal pass ((s + 512) >> 10 of four
// taps, packed two int16 a word) and the vertical pass (four 8-byte LDS reads, 16 __mul24, >> 10).  All three were shared functions
// first and measurably slower that way on an MI355X (profiles/upscale_refactor_ab.txt): the horizontal pass's five LDS reads are
// merged differently (up to 31 % on a 4K frame), the vertical pass costs the fp32 colour export 4 - 5 %, the luma load the r = 2
// int8 I420 video export 1.3 %.  A change to one of the six bodies belongs in its twin.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sesrq_chroma {

constexpr int HALO = 2;                       // staged LR samples around a tile, each side
constexpr int SEG = 16;                       // output values per lane and run

// The Keys a = -1/2 weights x 1024 of phase phi (rows) and the offset of tap 0 from j; r = 4: rows 0 .. 3, r = 2: rows 4, 5 of
// include/sesrq_colour.h's table.
__host__ __device__ constexpr int weight(int r, int phi, int k) {
    constexpr int W4[4][4] = {{-45, 399, 745, -75}, {-7, 93, 987, -49}, {-49, 987, 93, -7}, {-75, 745, 399, -45}};
    constexpr int W2[2][4] = {{-24, 232, 888, -72}, {-72, 888, 232, -24}};
    return r == 4 ? W4[phi][k] : W2[phi][k];
}
__host__ __device__ constexpr int first_tap(int r, int phi) { return 2 * phi < r ? -2 : -1; }

// the weight of tap k of a lane's own phase
template <int R>
__device__ inline int weight_of(int phi, int k) {
    int w = weight(R, 0, k);
#pragma unroll
    for (int q = 1; q < R; ++q) w = phi == q ? weight(R, q, k) : w;
    return w;
}

__device__ inline int half_of(unsigned w, int hi) { return hi ? (int)w >> 16 : (int)(short)(w & 0xffffu); }

// Words of a row of the horizontal pass that holds `cols` output columns, two a word.  cols / 2 is a power of two, which would put
// the same run of every row on the same banks; two words more and the rows a half wave reads together start two banks apart, so
// that e.g. the colour export's 4 rows x 8 runs of 8-byte reads fill the 64 banks.
constexpr int hwords(int cols) { return cols / 2 + 2; }

}  // namespace sesrq_chroma
