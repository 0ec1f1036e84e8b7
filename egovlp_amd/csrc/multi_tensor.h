// The work list of the multi-tensor launches: one workgroup per (item, block-sized piece of it), the items' pointers and sizes in a
// table that travels in the kernel arguments.  Three things: the index part of such a table, the device-side lookup "which item,
// which block of it, is blockIdx.x", and the host-side loop that validates a list, fills tables and launches them.
// The host part is plain C++ (tests/test_multi_tensor_cpu.py compiles it on its own).
#pragma once
#include <stdint.h>

// A table struct keeps its own pointer / size arrays and has a member `MtIndex<MAX_T> ix`.
template <int MAX_T>
struct MtIndex {
  static constexpr int capacity = MAX_T;
  int blk_start[MAX_T + 1];   // first block of each item (prefix sum of the block counts); blk_start[count] = the grid
  int count;
};

#ifdef __HIPCC__
struct MtWork {
  int item, block;            // block: index inside the item
};
// the last item with blk_start <= blockIdx.x: a binary search on scalars (<= 7 steps for the largest table)
template <int MAX_T>
__device__ __forceinline__ MtWork mt_locate(const MtIndex<MAX_T>& ix) {
  int lo = 0, hi = ix.count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)blockIdx.x >= ix.blk_start[mid]) lo = mid; else hi = mid - 1;
  }
  return {lo, (int)blockIdx.x - ix.blk_start[lo]};
}
#endif

// blocks(i)          -> block count of item i: 0 = skip it, negative = invalid
// fill(t, slot, i)      writes item i's fields into slot `slot` of the table
// launch(t, nb)      -> enqueues one kernel on nb blocks; 0 or an error code
// Every item is validated before the first launch: 1 (invalid argument) with nothing enqueued if any block count is negative or
// above 2^31 - 1.  A launch is started when the table is full or the next item would push its grid past 2^31 - 1 blocks.
// -> the first non-zero result of `launch`, else 0.
template <typename Table, typename Blocks, typename Fill, typename Launch>
int mt_for_each_launch(int count, Blocks blocks, Fill fill, Launch launch) {
  constexpr int MAX_T = decltype(Table::ix)::capacity;
  constexpr int64_t MAX_GRID = 0x7fffffff;
  for (int i = 0; i < count; ++i) {
    const int64_t b = blocks(i);
    if (b < 0 || b > MAX_GRID) return 1;
  }
  Table t;
  int nt = 0;
  int64_t nb = 0;
  auto flush = [&]() -> int {
    if (nt == 0) return 0;
    t.ix.blk_start[nt] = (int)nb;
    t.ix.count = nt;
    const int rc = launch(t, (int)nb);
    nt = 0;
    nb = 0;
    return rc;
  };
  for (int i = 0; i < count; ++i) {
    const int64_t b = blocks(i);
    if (b == 0) continue;
    if (nt == MAX_T || nb + b > MAX_GRID) {
      const int rc = flush();
      if (rc) return rc;
    }
    fill(t, nt, i);
    t.ix.blk_start[nt] = (int)nb;
    nb += b;
    ++nt;
  }
  return flush();
}
