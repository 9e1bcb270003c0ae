// rfx_blocks.h — the column-block map of the bounded gathers' row masks (include/rfx.h rfx_ssgi_hit_mask): a frame row is cut into 32 blocks,
// one bit each in the row's mask word.  The ONE statement of the map for the kernels that set the bits (k1_hit_mask, k6_name), the kernels
// that move the blocks (hist_pack_rows, peer_pull) and the host plan that sizes the messages (rfx_comm.hip).  0 <= x < W, 0 <= b <= 32, W < 2^23.
#pragma once
#include <hip/hip_runtime.h>

__host__ __device__ inline int rfx_block_of_col(int x, int W) { return (int)((unsigned int)(x * 32) / (unsigned int)W); }  // the block texel x is in
__host__ __device__ inline int rfx_block_col0(int b, int W) { return (int)((unsigned int)(b * W + 31) / 32u); }             // the first texel of block b
