// The rank arithmetic of the one-pass hash sort's scatter (deflate.hip: k_op_scatter), kept apart from the kernel so that a host
// program can replay it (tests/scatter_rank_check.cpp): no HIP in here beyond the function attributes.
//
// A wave counts its keys per bucket in 16-bit halves, buckets 2 j and 2 j + 1 sharing word j of the wave's row.  The counting
// atomic RETURNS the word as it was: the key's half of it is the number of the wave's earlier keys in that bucket -- its rank
// among them, because the LDS retires the lanes of one instruction in lane order and a wave's instructions in program order.
// After the workgroup's scan has turned the row into the wave's first places, a key's place in the slice is  start + rank.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define OP_RANK_FN __host__ __device__ inline
#else
#define OP_RANK_FN inline
#endif

namespace mts {

constexpr int OP_ID_BITS = 10;                       // a bucket number (< 1024) and its key's rank (< 512) share a register

OP_RANK_FN uint32_t op_cw_word(uint32_t id) { return id >> 1; }
OP_RANK_FN uint32_t op_cw_shift(uint32_t id) { return 16u * (id & 1u); }
OP_RANK_FN uint32_t op_cw_one(uint32_t id) { return 1u << op_cw_shift(id); }
// bucket and rank from the word the counting atomic returned
OP_RANK_FN uint32_t op_pack_rank(uint32_t id, uint32_t old_word) { return id | (((old_word >> op_cw_shift(id)) & 0xffffu) << OP_ID_BITS); }
OP_RANK_FN uint32_t op_rank_id(uint32_t idr) { return idr & ((1u << OP_ID_BITS) - 1u); }
// the key's place in the slice from the scanned word (the wave's first places of the two buckets)
OP_RANK_FN uint32_t op_slot(uint32_t idr, uint32_t start_word) { return ((start_word >> op_cw_shift(op_rank_id(idr))) & 0xffffu) + (idr >> OP_ID_BITS); }

}  // namespace mts
