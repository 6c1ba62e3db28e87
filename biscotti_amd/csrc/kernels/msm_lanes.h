// Lane map of the share MSM (msm.hip k_shares_msm): which (row position, chunk, slot) a lane of the grid
// computes.  A pure function of integers, plain C++ for host and device, so the order in which work reaches
// the GPU can be checked on the CPU (csrc/selftest): every (pos, k, slot) is hit exactly once.
#pragma once
#include "fixed_base.h"   // BSC_HD

constexpr int SHARE_MSM_THREADS = 256;   // lanes per block of the share MSM
constexpr int SHARE_MSM_SUPER = 64;      // blocks per super-block of the grouped order

// bijective on [0, nblocks): blocks that share an XCD (bid % 8) get a contiguous logical range
BSC_HD inline int xcd_remap(int bid, int nblocks) {
  const int q = nblocks / 8, r = nblocks % 8;
  const int xcd = bid % 8, idx = bid / 8;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}

struct ShareLane {
  int pos;     // position in the (compacted) row list, < neff
  int k;       // chunk, < nchunks
  int slot;    // lane of the (row, chunk) group, < SL
  bool none;   // surplus lane of the grid: nothing to do
};

// Lane `thread` of block `block` in a grid of `grid` blocks, over neff rows x nchunks chunks x SL lanes.
// group_rows G > 0: rows are taken G at a time in list order (the speculative rows arrive sorted by their
// arrival at the leader), chunk-major inside a group, and the XCD remap is applied per 64-block
// super-block -- so work proceeds through the row list in dispatch order (rows the selection drops later
// are skipped when reached) while each XCD still shares a chunk's table lines across the group's rows.
// G = 0: one group of every row, remapped over the whole grid.
BSC_HD inline ShareLane share_lane(int block, int thread, int grid, int neff, int nchunks, int SL, int group_rows) {
  ShareLane l{0, 0, 0, true};
  const long long total = (long long)neff * nchunks * SL;
  int lb;
  if (group_rows > 0) {
    const int q = (unsigned)block / SHARE_MSM_SUPER, j = (unsigned)block % SHARE_MSM_SUPER;   // block >= 0
    const int left = grid - q * SHARE_MSM_SUPER;
    lb = q * SHARE_MSM_SUPER + xcd_remap(j, left < SHARE_MSM_SUPER ? left : SHARE_MSM_SUPER);
  } else {
    lb = xcd_remap(block, grid);
  }
  const long long g = (long long)lb * SHARE_MSM_THREADS + thread;
  if (g >= total) return l;
  const int G = group_rows > 0 && group_rows < neff ? group_rows : neff;
  const long long per_group = (long long)G * nchunks * SL;
  const int gq = (int)(g / per_group);
  const int r0 = gq * G, gr = neff - r0 < G ? neff - r0 : G;
  const long long gg = g - (long long)gq * per_group;
  // chunk-major inside the group: consecutive groups of SL lanes share a chunk (and its table lines)
  l.slot = (int)(gg % SL);
  const long long grp = gg / SL;
  l.pos = r0 + (int)(grp % gr);
  l.k = (int)(grp / gr);
  l.none = false;
  return l;
}
