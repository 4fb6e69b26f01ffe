// Workgroup -> (channel, frequency hypothesis) tile of the scan and softbits kernels, one map for both.
//
// Workgroups are dealt round-robin over the 8 XCDs (GPU dies, each with its own L2), so each XCD gets one contiguous range of
// tiles.  Inside the range tiles are ordered in groups of G channels, frequency outer and channel inner: the ~96 tiles resident on
// an XCD then read G windows and 96 / G rows of the phasor table (mix.h), under 1 MB for G = 4..16, and every row meets its G
// readers while it is still in L2.  G = 1 is the plain order, channel outer and frequency inner.
// Plain C++ besides the two attributes: tests/test_mix_table_model.py compiles it with the host compiler.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MSK144_TILE_FN __host__ __device__ inline
#else
#define MSK144_TILE_FN inline
#endif

#ifndef MSK144_TILE_GROUP
#define MSK144_TILE_GROUP 8
#endif

namespace msk144
{

constexpr int kTileGroup = MSK144_TILE_GROUP;  // G; -DMSK144_TILE_GROUP=n builds a variant (tools/ab_variants.py)
static_assert(kTileGroup >= 1, "channels per tile group");

struct Tile
{
    int ch_rel;  // channel inside the block [ch0, ch0 + nch) the launch covers
    int b;       // frequency hypothesis
};

// tile t of nch x F: group t / (G F); inside it b = r / Gc, channel = r % Gc with Gc the group's size (the last one may be short)
template<int G = kTileGroup>
MSK144_TILE_FN Tile tile_of(int t, int nch, int F)
{
    const int group = t / (G * F);
    const int r = t - group * (G * F);
    const int left = nch - group * G;
    const int gc = left < G ? left : G;
    const int b = r / gc;
    return Tile{group * G + (r - b * gc), b};
}

// tiles per XCD of a launch over `total` tiles; the grid is 8 times this
MSK144_TILE_FN int tiles_per_xcd(int total)
{
    return (total + 7) / 8;
}

// the tile of workgroup `block` (blockIdx.x), or -1 for the surplus workgroups of the last XCD's range
MSK144_TILE_FN int tile_index(int block, int total)
{
    const int per_xcd = tiles_per_xcd(total);
    const int tile = (block & 7) * per_xcd + (block >> 3);
    return tile < total ? tile : -1;
}

}  // namespace msk144
