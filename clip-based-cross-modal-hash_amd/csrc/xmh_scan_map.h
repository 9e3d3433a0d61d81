// The block map of the scan launches: blockIdx -> (chunk, tile) and the grid that goes with it, for the host (launch_geom) and for every
// kernel that walks (chunk, tile) pairs -- k_scan_touch, both passes on the matrix cores, the VALU kernels.
//
// Block b runs on XCD b % 8 (observed, speed only).  Whole groups of 8 chunks: chunk c is pinned to XCD c % 8 and its tiles are swept
// back to back, so that the chunk's packed words stay in that XCD's L2 -- b & 7 is the XCD, t = b >> 3, tile t % ntile, chunk
// xcd + 8 (t / ntile).  The nchunk % 8 chunks left over follow as ntile further blocks each: consecutive blocks, and with them
// consecutive XCDs, take consecutive tiles of one chunk.  A leftover chunk is read through all eight L2s (about 100 KB per chunk at the
// headline shape; each L2 holds the whole packed gallery of that shape), and no XCD gets a chunk's worth of blocks more than another:
// nchunk need not be a multiple of 8 for the blocks of a launch to be spread evenly.  Every block of the grid has work.
#pragma once

namespace xmh {

__host__ __device__ inline unsigned scan_grid_blocks(int ntile, int nchunk) { return (unsigned)ntile * (unsigned)nchunk; }

__host__ __device__ inline bool scan_block_map(int b, int ntile, int nchunk, int& chunk_id, int& tile) {
    const int whole = nchunk & ~7;                       // chunks in whole groups of 8
    const int lb = b - whole * ntile;
    if (lb < 0) {
        const int t = b >> 3;
        tile = t % ntile;
        chunk_id = (b & 7) + 8 * (t / ntile);
        return true;
    }
    tile = lb % ntile;
    chunk_id = whole + lb / ntile;
    return chunk_id < nchunk;
}

}  // namespace xmh
