// What tests/blockwalk_san.cpp and tests/blockcycle_san.cpp share: a run and its generator, one tile of
// a scan driven lane by lane through blockwalk_dev.h's tile rules (the text both scan kernels
// compile), the roll, and the walk's sequential form, which the cycle's program holds its own
// against on runs without a transition block.  Plain C++ for g++ under ASan+UBSan.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../blockwalk_dev.h"

namespace san {

using namespace pz;

constexpr uint64_t kTile = kBwTile, kWave = 64, kWaves = kBwWaves;

struct Run {
  uint64_t n = 0, has0 = 0, cslot0 = 0, lsr = 0, lag = 0;
  uint32_t flags = 0;  // the gate's flag word
  std::vector<uint64_t> slot;
  std::vector<uint8_t> report, hash;  // n, n x 32
  std::vector<uint8_t> ring, ring_len;  // 129 x 32, 129
  std::vector<uint32_t> att_block;
  std::vector<uint64_t> parents_start;
  std::vector<uint8_t> pend_take;
  std::vector<int32_t> vote_status;
};

inline std::mt19937_64 rng;  // (a program seeds it before its first case)

template <class T>
void same(const std::vector<T>& a, const std::vector<T>& b, const char* what, const char* name) {
  if (a == b) return;
  size_t i = 0;
  while (i < a.size() && i < b.size() && a[i] == b[i]) ++i;
  std::printf("FAIL %s: %s differs at %zu (sizes %zu, %zu)\n", name, what, i, a.size(), b.size());
  std::exit(1);
}

// go: 0 none, 1 all, 2 alternating, 3 random.  slot_of gives block j's slot.
template <class F>
Run make(uint64_t n, int go, F slot_of, uint64_t has0, uint64_t cslot0, uint64_t lsr, uint64_t lag) {
  Run r;
  r.n = n, r.has0 = has0, r.cslot0 = cslot0, r.lsr = lsr, r.lag = lag;
  r.flags = rng() % 8 == 0;
  r.slot.resize(n), r.report.resize(n), r.hash.resize(32 * n);
  for (uint64_t j = 0; j < n; ++j) {
    r.slot[j] = slot_of(j);
    r.report[j] = go == 0 ? 0 : go == 1 ? 1 + j % 2 : go == 2 ? j % 2 : (rng() % 4 ? 1 + rng() % 2 : 0);
  }
  for (auto& b : r.hash) b = (uint8_t)rng();
  r.ring.resize(kBwRing * 32), r.ring_len.resize(kBwRing);
  for (auto& b : r.ring) b = (uint8_t)rng();
  for (auto& l : r.ring_len) l = rng() % 3 ? 32 : (uint8_t)(rng() % 33);
  for (uint64_t j = 0; j < n; ++j)
    for (uint64_t k = rng() % 4; k > 0; --k) {
      r.att_block.push_back((uint32_t)j);
      r.parents_start.push_back(rng() % 65);
      r.pend_take.push_back(rng() % 2);
      r.vote_status.push_back((int32_t)(rng() % 3 ? PZ_ATT_PROCESSED : rng() % 8));
    }
  return r;
}

// One tile behind round 1: every lane's inputs and its bw_round1, and the candidates' ballot words.
struct Tile {
  bool go[kTile];
  uint64_t slot[kTile], cb[kWaves];
  BwRound1 r1[kTile];
};

// A ballot word a wave: bit l of words[w] is whether lane 64 w + l is a candidate whose slot has pred.
template <class P>
void ballot(const Tile& t, uint64_t* words, P pred) {
  for (uint64_t w = 0; w < kWaves; ++w) {
    words[w] = 0;
    for (uint64_t l = 0; l < kWave; ++l)
      if (t.r1[w * kWave + l].cand && pred(t.slot[w * kWave + l])) words[w] |= 1ull << l;
  }
}

// Round 1 as scan_round1 (blockscan_wave.h) takes it: the waves' words a lane at a time, then
// bw_round1 for every lane.  What the kernels keep as tile-uniform must be the same in every lane.
inline void round1(const Run& r, const BwCarry& c, uint64_t t0, Tile& t) {
  uint64_t before[kTile], s_max[kWaves], s_fslot[kWaves];
  uint32_t s_fgo[kWaves];
  for (uint64_t w = 0; w < kWaves; ++w) {
    uint64_t inc = 0;
    s_fgo[w] = 64, s_fslot[w] = 0;
    for (uint64_t l = 0; l < kWave; ++l) {
      const uint64_t i = w * kWave + l, j = t0 + i;
      t.go[i] = j < r.n && bw_go(r.report[j]);
      t.slot[i] = j < r.n ? r.slot[j] : 0;
      before[i] = inc;
      const uint64_t v = bw_scan_value(t.go[i], true, t.slot[i]);
      if (v > inc) inc = v;
      if (t.go[i] && s_fgo[w] == 64) s_fgo[w] = (uint32_t)l, s_fslot[w] = t.slot[i];
    }
    s_max[w] = inc;
  }
  for (uint64_t i = 0; i < kTile; ++i) {
    t.r1[i] = bw_round1(c, s_max, s_fgo, s_fslot, before[i], t0, (uint32_t)(i / kWave), t0 + i, t.go[i], t.slot[i]);
    if (t.r1[i].tile_max != t.r1[0].tile_max || t.r1[i].first != t.r1[0].first) {
      std::printf("FAIL: lane %llu of the tile at %llu has its own tile_max or first\n", (unsigned long long)i, (unsigned long long)t0);
      std::exit(1);
    }
  }
  ballot(t, t.cb, [](uint64_t) { return true; });
}

// Round 2 for lane i: its rank, and the tile's count, which the kernels keep as tile-uniform too.
inline BwRank rank_of(const BwCarry& c, const Tile& t, uint64_t i) {
  const BwRank k = bw_rank(c, t.cb, (uint32_t)i);
  if (k.tile_cnt != bw_rank(c, t.cb, 0).tile_cnt) {
    std::printf("FAIL: lane %llu of a tile has its own tile count\n", (unsigned long long)i);
    std::exit(1);
  }
  return k;
}

// The roll kernel: the ring after ncand candidates went into the log.
inline void roll(const Run& r, const std::vector<uint8_t>& log, uint64_t ncand, std::vector<uint8_t>& ring, std::vector<uint8_t>& ring_len) {
  std::vector<uint8_t> to(kBwRing * 32), to_len(kBwRing);
  const uint64_t nroll = bw_roll_count(ncand, r.flags);
  for (uint64_t k = 0; k < kBwRing; ++k) {
    std::memcpy(&to[32 * k], &log[32 * bw_roll_src(k, nroll)], 32);
    to_len[k] = bw_roll_len(r.ring_len[k], nroll);
  }
  ring = to, ring_len = to_len;
}

// ---- the walk's kernels, lane by lane --------------------------------------------------------------
struct WalkOut {
  std::vector<uint8_t> walk, log, ring, ring_len, pend_take;
  std::vector<uint64_t> base, parents_start;
  std::vector<int32_t> vote_status;
  uint64_t result[kBwResultWords] = {};
};

inline WalkOut walk_sequential(const Run& r) {
  WalkOut o;
  const uint64_t n = r.n;
  o.walk.assign(n, 0xEE);
  o.base.assign(n, 0xEEEE);
  o.log.assign((kBwRing + n) * 32, 0xEE);
  o.ring = r.ring, o.ring_len = r.ring_len;
  o.parents_start = r.parents_start, o.pend_take = r.pend_take, o.vote_status = r.vote_status;
  if (n == 0) {  // nothing is launched; the host form's record
    o.result[kBwHasCandidate] = r.has0 != 0, o.result[kBwCandidateSlot] = r.has0 ? r.cslot0 : 0;
    o.log = r.ring;
    return o;
  }
  // scan
  std::memcpy(o.log.data(), r.ring.data(), kBwRing * 32);
  BwCarry c = bw_carry(r.has0, r.cslot0);
  bool fin_set = false;
  uint64_t c_stop = kBwNone, fin[3] = {};
  for (uint64_t t0 = 0; t0 < n; t0 += kTile) {
    if (c_stop != kBwNone) {
      for (uint64_t j = t0; j < n && j < t0 + kTile; ++j) o.walk[j] = kBwDeferred, o.base[j] = 0;
      continue;
    }
    Tile t;
    uint64_t tb[kWaves];
    round1(r, c, t0, t);
    ballot(t, tb, [&r](uint64_t slot) { return bw_transition(slot, r.lsr); });  // round 2
    const uint64_t stop = bw_tile_stop(c, t0, r.lag, n, t.cb, tb);
    uint64_t stop_by_rule = kBwNone, tile_cnt = 0;
    for (uint64_t i = 0; i < kTile && t0 + i < n; ++i) {
      const uint64_t j = t0 + i;
      const BwRound1& x = t.r1[i];
      const BwRank k = rank_of(c, t, i);
      // (the per-block statement of the stop, which the tile's must equal)
      const uint64_t s = bw_stop_at(j, x.cand, k.rank, t.slot[i], r.lsr, r.lag);
      if (s < stop_by_rule) stop_by_rule = s;
      const bool deferred = j >= stop;
      o.walk[j] = bw_walk(t.go[i], x.cand, deferred);
      o.base[j] = bw_base(r.lag, k.rank, deferred);
      if (x.cand && !deferred) std::memcpy(&o.log[32 * (kBwRing + k.rank)], &r.hash[32 * j], 32);
      if (j == stop) fin[0] = k.rank, fin[1] = x.pending, fin[2] = x.before, fin_set = true;
      tile_cnt = k.tile_cnt;
    }
    if ((stop_by_rule >= n ? kBwNone : stop_by_rule) != stop) {
      std::printf("FAIL: tile stop %llu, by rule %llu\n", (unsigned long long)stop, (unsigned long long)stop_by_rule);
      std::exit(1);
    }
    c_stop = stop;
    bw_advance(c, t.r1[0], tile_cnt);
  }
  const uint64_t ncand = fin_set ? fin[0] : c.cnt;
  o.result[kBwStop] = c_stop == kBwNone ? n : c_stop;
  o.result[kBwNcand] = ncand;
  o.result[kBwHasCandidate] = fin_set ? fin[1] : (uint64_t)c.pending;
  o.result[kBwCandidateSlot] = fin_set ? fin[2] : c.max;
  for (uint64_t p = 32 * (kBwRing + ncand); p < 32 * (kBwRing + n); ++p) o.log[p] = 0;
  // rows
  for (size_t i = 0; i < r.att_block.size(); ++i) {
    const uint64_t b = r.att_block[i];
    if (b >= n) continue;
    const BwRow x = bw_row(o.parents_start[i], o.pend_take[i], o.vote_status[i], o.walk[b], o.base[b]);
    o.parents_start[i] = x.parents_start, o.pend_take[i] = x.pend_take, o.vote_status[i] = x.vote_status;
  }
  roll(r, o.log, ncand, o.ring, o.ring_len);
  return o;
}

}  // namespace san
