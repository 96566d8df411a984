// placement_main.cpp -- stand-alone check of csrc/rex_placement.h: which envs of a REX_TASK_MIXED batch share a wave, run on the
// host without the library (tests/test_host_and_abi.py compiles it with the address and undefined-behaviour sanitizers and runs it).
// Exit status 0: every case holds; 1 and a line on stderr per failed property otherwise.
#include "rex_placement.h"

#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Case { int n, epw, base; uint32_t seed; int n_mix; int32_t mix[3]; };

static void check_case(const Case& c) {
  const int n = c.n, epw = c.epw;
  int32_t mix_task[5];
  for (int k = 0; k < 5; ++k) mix_task[k] = c.mix[k < c.n_mix ? k : 0];   // (the library fills the unused entries with the first task)
  const std::vector<int32_t> cls = rex::mixed_classes(n, c.base, c.seed, 0u, c.n_mix);
  CHECK((int)cls.size() == n, "n=%d", n);
  for (int i = 0; i < n; ++i) {   // cls[i]: the index in mix_task of the env's drawn task
    const int k = rex::mixed_task_draw(c.seed, 0u, c.base + i, c.n_mix);
    CHECK(k >= 0 && k < c.n_mix && cls[i] == k, "n=%d env %d: class %d, draw %d", n, i, (int)cls[i], k);
  }

  // ---- the chunked map ----
  {
    std::vector<int32_t> slots, tasks;
    const int busy = rex::task_slot_map(cls, c.n_mix, mix_task, epw, slots, tasks);
    CHECK(tasks.size() * (size_t)epw == slots.size(), "n=%d epw=%d: %zu blocks, %zu slots", n, epw, tasks.size(), slots.size());
    std::vector<int> seen((size_t)n, 0);
    int holding = 0;
    for (size_t b = 0; b < tasks.size(); ++b) {
      bool any = false;
      for (int k = 0; k < epw; ++k) {
        const int32_t e = slots[b * epw + k];
        if (e < 0) { CHECK(e == -1, "n=%d block %zu slot %d: padding %d", n, b, k, (int)e); continue; }
        CHECK(e < n, "n=%d block %zu slot %d: env %d", n, b, k, (int)e);
        if (e >= n) continue;
        any = true;
        ++seen[(size_t)e];
        CHECK(mix_task[cls[(size_t)e]] == tasks[b], "n=%d block %zu of task %d holds env %d of task %d", n, b, (int)tasks[b], (int)e, (int)mix_task[cls[(size_t)e]]);
      }
      holding += any;
    }
    for (int i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1, "n=%d epw=%d: env %d placed %d times", n, epw, i, seen[(size_t)i]);
    CHECK(busy == holding, "n=%d epw=%d: busy %d, %d blocks hold an env", n, epw, busy, holding);
    bool tail = false;   // does the last workgroup hold an env?
    for (int k = 0; k < epw && !tasks.empty(); ++k) tail = tail || slots[(tasks.size() - 1) * epw + k] >= 0;
    CHECK(tail, "n=%d epw=%d: a trailing padding workgroup remains", n, epw);
  }

  // ---- the region map ----
  {
    std::vector<int32_t> slots, tasks;
    int32_t base[5] = {-7, -7, -7, -7, -7};
    rex::task_region_map(cls, c.n_mix, mix_task, epw, slots, tasks, base);
    CHECK(tasks.size() * (size_t)epw == slots.size(), "n=%d epw=%d: %zu blocks, %zu slots", n, epw, tasks.size(), slots.size());
    for (int k = c.n_mix; k < 5; ++k) CHECK(base[k] == 0, "n=%d: base[%d] = %d of an unused class", n, k, (int)base[k]);
    CHECK(base[0] == 0, "n=%d: base[0] = %d", n, (int)base[0]);
    for (int k = 0; k < c.n_mix; ++k) {
      const size_t begin = (size_t)base[k], end = k + 1 < c.n_mix ? (size_t)base[k + 1] : slots.size();
      CHECK(base[k] >= 0 && base[k] % epw == 0 && begin <= end && end <= slots.size(), "n=%d: region %d = [%zu, %zu) of %zu", n, k, begin, end, slots.size());
      if (!(base[k] >= 0 && begin <= end && end <= slots.size())) continue;
      size_t s = begin;
      for (int i = 0; i < n; ++i)   // the envs of class k in ascending order ...
        if (cls[(size_t)i] == k) { CHECK(s < end && slots[s] == i, "n=%d region %d slot %zu: want env %d", n, k, s, i); ++s; }
      CHECK(end - s < (size_t)epw, "n=%d region %d: %zu padding slots", n, k, end - s);   // ... then fewer than epw slots of -1
      for (; s < end; ++s) CHECK(slots[s] == -1, "n=%d region %d slot %zu: padding %d", n, k, s, (int)slots[s]);
      for (size_t b = begin / epw; b < end / epw; ++b) CHECK(tasks[b] == mix_task[k], "n=%d block %zu of region %d: task %d", n, b, k, (int)tasks[b]);
    }
  }
}

int main() {
  // Philox4x32-10 known answers (Random123's kat_vectors): zeros, all ones, the digits of pi
  const uint32_t kat[3][10] = {
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
    {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
    {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
  for (const auto& v : kat) {
    uint32_t ctr[4] = {v[0], v[1], v[2], v[3]};
    rex::philox4x32(ctr, v[4], v[5]);
    for (int k = 0; k < 4; ++k) CHECK(ctr[k] == v[6 + k], "philox4x32 word %d: %08x, want %08x", k, (unsigned)ctr[k], (unsigned)v[6 + k]);
  }
  const int32_t WALK = 0, GALLOP = 1, TURN = 2;   // include/rexsim.h REX_TASK_*
  const Case cases[] = {
    {96, 4, 0, 4u, 3, {WALK, GALLOP, TURN}},   {2048, 4, 0, 0u, 3, {WALK, GALLOP, TURN}}, {2048, 4, 6144, 0u, 3, {WALK, GALLOP, TURN}},
    {5000, 8, 0, 4u, 3, {WALK, GALLOP, TURN}}, {16384, 16, 0, 0u, 3, {WALK, GALLOP, TURN}}, {1, 4, 0, 1u, 3, {WALK, GALLOP, TURN}},
    {37, 16, 5, 2u, 3, {WALK, GALLOP, TURN}},  {37, 16, 5, 2u, 2, {GALLOP, TURN, 0}},      {37, 16, 5, 2u, 1, {TURN, 0, 0}}};
  for (const Case& c : cases) check_case(c);
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  printf("placement: %zu cases hold\n", sizeof cases / sizeof cases[0]);
  return 0;
}
