// rex_placement.h -- which envs of a REX_TASK_MIXED batch share a wave: plain host code (standard headers and rex_philox.h only),
// so that a program without a GPU can run it (tests/placement_main.cpp).
//
// An env of a mixed batch keeps the task drawn for it (rex::mixed_task_draw: one Philox block keyed by the seed and the global
// env index) for its whole life, so which envs share a wave is decided ONCE: the envs are cut into chunks of neighbouring
// indices (their state words share 64-byte sectors), a chunk's envs are sorted by task, every task's run is padded to whole
// waves, and the chunks' workgroups are dealt to the XCDs (workgroup b runs on XCD b % 8) so that one L2 fetches a chunk's
// sectors.  The step kernel then runs waves of ONE task: action_repeat, sweep cap, action box and reward weight are
// wave-uniform, a 5-substep wave does not sit through gallop's sixth substep, and the kernel is the single-task kernel.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "rex_philox.h"

namespace rex {

// cls[i] = the task slot (index into the mix) drawn for env i of a batch whose first env has the global index env_index_base
inline std::vector<int32_t> mixed_classes(int n, int env_index_base, uint32_t seed_lo, uint32_t seed_hi, int n_mix) {
  std::vector<int32_t> cls((size_t)n);
  for (int i = 0; i < n; ++i) cls[(size_t)i] = mixed_task_draw(seed_lo, seed_hi, env_index_base + i, n_mix);
  return cls;
}

// slots[blk * epw + k] = env of wave slot k of workgroup blk (-1: padding), tasks[blk] = the workgroup's task
// returns the number of workgroups that hold envs (the others leave at once)
inline int task_slot_map(const std::vector<int32_t>& cls, int n_mix, const int32_t mix_task[5], int epw, std::vector<int32_t>& slots,
                         std::vector<int32_t>& tasks) {
  const int n = (int)cls.size();
  // 8 m chunks of whole sectors (m per XCD), each at most 64 waves' worth: padding <= (epw - 1) slots per task and chunk
  const int m = (n + 8 * 64 * epw - 1) / (8 * 64 * epw);
  const int chunk = ((n + 8 * m - 1) / (8 * m) + 15) / 16 * 16;
  const int nchunks = (n + chunk - 1) / chunk;
  std::vector<std::vector<int32_t>> xs(8), xt(8);    // per XCD: its workgroups' slots and tasks
  for (int c = 0; c < nchunks; ++c) {
    std::vector<int32_t>& s = xs[c & 7];
    for (int k = 0; k < n_mix; ++k) {
      const size_t before = s.size();
      for (int i = c * chunk; i < n && i < (c + 1) * chunk; ++i)
        if (cls[(size_t)i] == k) s.push_back(i);
      while ((s.size() - before) % (size_t)epw) s.push_back(-1);
      for (size_t b = before / epw; b < s.size() / epw; ++b) xt[c & 7].push_back(mix_task[k]);
    }
  }
  size_t rounds = 0, busy = 0;
  for (int x = 0; x < 8; ++x) { busy += xt[x].size(); if (xt[x].size() > rounds) rounds = xt[x].size(); }
  slots.assign(rounds * 8 * (size_t)epw, -1);
  tasks.assign(rounds * 8, mix_task[0]);
  for (int x = 0; x < 8; ++x)
    for (size_t j = 0; j < xt[x].size(); ++j) {
      const size_t b = 8 * j + (size_t)x;
      tasks[b] = xt[x][j];
      for (int k = 0; k < epw; ++k) slots[b * epw + k] = xs[x][j * epw + k];
    }
  while (!tasks.empty() && slots[(tasks.size() - 1) * epw] < 0) { tasks.pop_back(); slots.resize(tasks.size() * epw); }   // trailing padding workgroups
  return (int)busy;
}

// The layout a regrouped mixed batch starts from (and keeps the shape of): task slot k's envs in index order in ONE region of
// whole waves per task, regions in the order of the mix; base[k] = first slot of region k.
inline void task_region_map(const std::vector<int32_t>& cls, int n_mix, const int32_t mix_task[5], int epw, std::vector<int32_t>& slots,
                            std::vector<int32_t>& tasks, int32_t base[5]) {
  const int n = (int)cls.size();
  slots.clear(); tasks.clear();
  for (int k = 0; k < 5; ++k) base[k] = 0;
  for (int k = 0; k < n_mix; ++k) {
    base[k] = (int32_t)slots.size();
    for (int i = 0; i < n; ++i) if (cls[(size_t)i] == k) slots.push_back(i);
    while (slots.size() % (size_t)epw) slots.push_back(-1);
    while (tasks.size() < slots.size() / epw) tasks.push_back(mix_task[k]);
  }
}

}  // namespace rex
