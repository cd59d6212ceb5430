// What the scan-fitting sources (scan.hip, align.hip, surface.hip) share: the live-row count of a body, the fp64 wave sum, the
// squared distance in its one fixed form and the split of a target range into chunks.
#pragma once
#include "sh_common.h"
#include <math.h>

constexpr int NN_WG_SLOTS = 2048;   // workgroups the chip holds at once (256 CUs x 8): the automatic split aims at this many

__device__ __forceinline__ int clamp_count(const int32_t* cnt, int b, int rows) {
    if (!cnt) return rows;
    const int c = cnt[b];
    return c < 0 ? 0 : (c > rows ? rows : c);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The distance of the header, in its one fixed form.
__device__ __forceinline__ float nn_d2(float qx, float qy, float qz, float tx, float ty, float tz) {
    const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}

// The split actually run for a request of `chunks` (0 = automatic: fill the chip) over nt targets in LDS tiles of `tile`, with
// `qt` queries per workgroup: whole tiles per chunk, no empty chunk.  Rounding the result once more changes nothing.
static inline int nn_resolve_chunks(int B, int nq, int nt, int tile, int qt, int chunks, int* tiles_per_chunk) {
    const int tiles = nt > 0 ? sh_cdiv(nt, tile) : 1;
    long c = chunks;
    if (c <= 0) {
        const long wgs = (long)sh_cdiv(nq > 0 ? nq : 1, qt) * (B > 0 ? B : 1);
        c = (NN_WG_SLOTS + wgs - 1) / wgs;
    }
    if (c > tiles) c = tiles;
    if (c < 1) c = 1;
    const int tpc = sh_cdiv(tiles, (int)c);
    *tiles_per_chunk = tpc;
    return sh_cdiv(tiles, tpc);
}
