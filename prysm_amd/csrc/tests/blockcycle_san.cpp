// The rules of a run across a cycle transition on the CPU under ASan+UBSan: blockcycle_dev.h (the
// inlines the kernels of blockcycle.hip compile too) driven through a sequential form of the scan
// kernel -- tiles of 1,024 lanes in waves of 64, the carry and the run's state between tiles, the
// two rounds a tile with their ballot words, every lane through the same bw_round1 / bw_rank /
// bc_tile / bw_advance the kernel calls -- and of the rows and roll kernels, against a plain
// restatement of blockchain/service.go:320-363 that walks block by block with a pending-candidate
// variable, a "the candidate's states are not promoted yet" flag, a last_state_recalc that advances
// at the transition block and a list that only grows (computeNewActiveState, core.go:223-237).
// On a run without a transition block the form must also give what the walk's form
// (walk_sequential, blockscan_san.h) gives.  Every array has exactly its size.  Prints counts; exit
// status 0 iff all agree.
#include "../blockcycle_dev.h"
#include "blockscan_san.h"

using namespace san;

namespace {

struct Out {
  std::vector<uint8_t> walk, log, ring, ring_len, take0, take1;
  std::vector<uint64_t> base, parents_start;
  std::vector<int32_t> vote0, vote1;
  uint64_t result[kBcResultWords] = {};
};

// ---- the reference, block by block ---------------------------------------------------------------
Out reference(const Run& r) {
  Out o;
  o.walk.assign(r.n, kBwDeferred);
  o.base.assign(r.n, 0);
  std::vector<uint8_t> list = r.ring, list_len = r.ring_len;  // a Go slice that is appended to
  bool has = r.has0 != 0;
  bool unpromoted = r.lag != 0;  // a transition block is the pending candidate: its states are not the chain's yet
  uint64_t lsr = r.lsr;          // LastStateRecalc of the state IsCycleTransition will read (core.go:181-183)
  uint64_t cslot = has ? r.cslot0 : 0, ncand = 0, stop = r.n, t = kBwNone, t_rank = 0, t_slot = 0;
  for (uint64_t j = 0; j < r.n; ++j) {
    // RecentBlockHashes() as this block reads it: the chain's, which lacks the transition block's hash
    o.base[j] = list_len.size() - kBwWindow - (unpromoted ? 1 : 0);
    if (r.report[j] == 0) {
      o.walk[j] = kBwOff;
      continue;
    }
    const bool had = has;
    if (has && r.slot[j] > cslot && r.slot[j] > 1) has = false;  // updateHead, service.go:320-322: the candidate's states are promoted
    if (has) {                                                   // :331-333
      o.walk[j] = kBwSaved;
      continue;
    }
    const bool was_unpromoted = unpromoted;
    if (r.slot[j] >= lsr + 64) {  // IsCycleTransition on the promoted state
      if (t != kBwNone) {         // a second stateRecalc: the next call's
        has = had, stop = j, o.base[j] = 0;
        break;
      }
      t = j, t_rank = ncand, t_slot = r.slot[j], lsr += 64;  // stateRecalc, core.go:398-497: new states for the candidate
      unpromoted = true;
    } else {
      unpromoted = false;
    }
    list.insert(list.end(), r.hash.begin() + 32 * j, r.hash.begin() + 32 * j + 32);  // core.go:230-237
    list_len.assign(list_len.size() + 1, 32);  // RecentBlockHashes() is the [32]byte form of every entry, stored back whole
    has = true, cslot = r.slot[j], ++ncand;  // service.go:361
    o.walk[j] = kBwCandidate;
    if (was_unpromoted) {  // this block promoted a transition block's states: the run ends behind it
      stop = j + 1;
      break;
    }
  }
  o.result[kBwStop] = stop, o.result[kBwNcand] = ncand, o.result[kBwHasCandidate] = has, o.result[kBwCandidateSlot] = cslot;
  o.result[kBcTIndex] = t, o.result[kBcTRank] = t_rank, o.result[kBcTSlot] = t_slot, o.result[kBcLagOut] = unpromoted;
  o.log = list;
  o.log.resize((kBwRing + r.n) * 32, 0);
  o.ring.assign(list.end() - kBwRing * 32, list.end());
  o.ring_len.assign(list_len.end() - kBwRing, list_len.end());
  if (r.flags & 1) o.ring = r.ring, o.ring_len = r.ring_len;  // a panic somewhere in the batch: nothing of it lands
  const size_t na = r.att_block.size();
  o.parents_start = r.parents_start, o.vote0.assign(na, 0), o.vote1.assign(na, 0), o.take0.assign(na, 0), o.take1.assign(na, 0);
  for (size_t i = 0; i < na; ++i) {
    const uint64_t b = r.att_block[i];
    const int32_t vs = r.vote_status[i], off = vs == PZ_ATT_PROCESSED ? PZ_ATT_NOT_PROCESSED : vs;
    const bool live = b < stop, after = t != kBwNone && b > t;  // tallied after stateRecalc
    if (live) o.parents_start[i] += o.base[b];
    o.vote0[i] = live && !after ? vs : off;
    o.vote1[i] = live && after ? vs : off;
    const bool cand = live && r.pend_take[i] && o.walk[b] == kBwCandidate;
    o.take0[i] = cand && (t == kBwNone || b < t);
    o.take1[i] = cand && t != kBwNone && b >= t;
  }
  return o;
}

// ---- the kernels, lane by lane ---------------------------------------------------------------------
Out sequential(const Run& r) {
  Out o;
  const uint64_t n = r.n, lag = r.lag, lsr_after = bc_lsr_after(r.lsr, lag);
  const size_t na = r.att_block.size();
  o.walk.assign(n, 0xEE);
  o.base.assign(n, 0xEEEE);
  o.log.assign((kBwRing + n) * 32, 0xEE);
  o.ring = r.ring, o.ring_len = r.ring_len;
  o.parents_start = r.parents_start;
  o.vote0.assign(na, 0xEE), o.vote1.assign(na, 0xEE), o.take0.assign(na, 0xEE), o.take1.assign(na, 0xEE);
  if (n == 0) {  // nothing is launched; the host form's record
    o.result[kBwHasCandidate] = r.has0 != 0, o.result[kBwCandidateSlot] = r.has0 ? r.cslot0 : 0;
    o.result[kBcTIndex] = kBwNone, o.result[kBcLagOut] = lag;
    o.log = r.ring;
    return o;
  }
  // scan
  std::memcpy(o.log.data(), r.ring.data(), kBwRing * 32);
  BwCarry c = bw_carry(r.has0, r.cslot0);
  uint64_t fin_rank = 0, fin_pending = 0, fin_before = 0, fin_slot = 0, fin_trank = 0, fin_tslot = 0;
  BcState st = bc_start(lag), by_rule = bc_start(lag);
  for (uint64_t t0 = 0; t0 < n; t0 += kTile) {
    if (st.stop != kBwNone) {
      for (uint64_t j = t0; j < n && j < t0 + kTile; ++j) o.walk[j] = kBwDeferred, o.base[j] = 0;
      continue;
    }
    Tile t;
    uint64_t tb[kWaves], ta[kWaves];
    round1(r, c, t0, t);
    ballot(t, tb, [&r](uint64_t slot) { return bw_transition(slot, r.lsr); });  // round 2: the ballot words
    ballot(t, ta, [lsr_after](uint64_t slot) { return bw_transition(slot, lsr_after); });
    bc_tile(st, t0, lag, t.cb, tb, ta);
    uint64_t tile_cnt = 0;
    for (uint64_t i = 0; i < kTile && t0 + i < n; ++i) {
      const uint64_t j = t0 + i;
      const BwRound1& x = t.r1[i];
      const BwRank k = rank_of(c, t, i);
      if (x.cand) bc_candidate(by_rule, j, t.slot[i], r.lsr, lag);  // (the per-block statement, which the tile's must equal)
      const bool deferred = bc_deferred(st, j);
      o.walk[j] = bw_walk(t.go[i], x.cand, deferred);
      o.base[j] = bc_base(bc_lagged(st, lag, j), k.rank, deferred);
      if (x.cand && !deferred) std::memcpy(&o.log[32 * (kBwRing + k.rank)], &r.hash[32 * j], 32);
      if (j == st.t_index) fin_trank = k.rank, fin_tslot = t.slot[i];
      if (j == st.l_index) fin_rank = k.rank, fin_pending = x.pending, fin_before = x.before, fin_slot = t.slot[i];
      tile_cnt = k.tile_cnt;
    }
    if (by_rule.t_index != st.t_index || by_rule.l_index != st.l_index || by_rule.stop != st.stop || by_rule.lag_out != st.lag_out) {
      std::printf("FAIL: tile state (%llu %llu %llu %llu), by rule (%llu %llu %llu %llu)\n", (unsigned long long)st.t_index,
                  (unsigned long long)st.l_index, (unsigned long long)st.stop, (unsigned long long)st.lag_out,
                  (unsigned long long)by_rule.t_index, (unsigned long long)by_rule.l_index, (unsigned long long)by_rule.stop,
                  (unsigned long long)by_rule.lag_out);
      std::exit(1);
    }
    bw_advance(c, t.r1[0], tile_cnt);
  }
  const bool met = st.l_index != kBwNone, included = met && st.stop == st.l_index + 1;
  const uint64_t ncand = met ? fin_rank + (included ? 1 : 0) : c.cnt;
  o.result[kBwStop] = st.stop == kBwNone ? n : st.stop;
  o.result[kBwNcand] = ncand;
  o.result[kBwHasCandidate] = included ? 1 : met ? fin_pending : (uint64_t)c.pending;
  o.result[kBwCandidateSlot] = included ? fin_slot : met ? fin_before : c.max;
  o.result[kBcTIndex] = st.t_index, o.result[kBcTRank] = fin_trank, o.result[kBcTSlot] = fin_tslot, o.result[kBcLagOut] = st.lag_out;
  for (uint64_t p = 32 * (kBwRing + ncand); p < 32 * (kBwRing + n); ++p) o.log[p] = 0;
  // rows
  for (size_t i = 0; i < na; ++i) {
    const uint64_t b = r.att_block[i];
    const bool named = b < n;
    const BcRow x = bc_row(o.parents_start[i], r.pend_take[i], r.vote_status[i], named ? o.walk[b] : kBwDeferred, named ? o.base[b] : 0, b,
                           o.result[kBcTIndex]);
    o.parents_start[i] = x.parents_start, o.vote0[i] = x.vote0, o.vote1[i] = x.vote1, o.take0[i] = x.take0, o.take1[i] = x.take1;
  }
  roll(r, o.log, ncand, o.ring, o.ring_len);
  return o;
}

uint64_t g_runs, g_blocks, g_deferred, g_saved, g_cands, g_rows, g_with_t, g_l_deferred, g_lag_t, g_after, g_walks, g_walks_lag, g_walks_early;

// A run in which no candidate at or before the walk's stop is a transition: the walk's form stops at
// the run's end, or with lag behind its one candidate (a transition candidate stops the walk before
// itself, with none taken under lag).  There the cycle's form must be the walk's: the same record,
// codes, bases, log and ring, phase 0 the walk's narrowed columns, phase 1 empty and no T.
void agree_with_walk(const Run& r, const Out& g, const char* name) {
  const WalkOut w = walk_sequential(r);
  if (!(w.result[kBwStop] == r.n || (r.lag && w.result[kBwNcand] == 1))) return;
  for (int k = 0; k < kBwResultWords; ++k)
    if (w.result[k] != g.result[k]) {
      std::printf("FAIL %s: result[%d] %llu, the walk's %llu\n", name, k, (unsigned long long)g.result[k], (unsigned long long)w.result[k]);
      std::exit(1);
    }
  if (r.n && g.result[kBcTIndex] != kBwNone) {
    std::printf("FAIL %s: t_index %llu on a run the walk takes whole\n", name, (unsigned long long)g.result[kBcTIndex]);
    std::exit(1);
  }
  std::vector<int32_t> narrowed = r.vote_status;
  for (auto& v : narrowed) v = bc_narrow(v);
  same(w.walk, g.walk, "walk (the walk's)", name);
  same(w.base, g.base, "base (the walk's)", name);
  same(w.log, g.log, "log (the walk's)", name);
  same(w.ring, g.ring, "ring (the walk's)", name);
  same(w.ring_len, g.ring_len, "ring lengths (the walk's)", name);
  same(w.parents_start, g.parents_start, "parents_start (the walk's)", name);
  if (r.n) {  // (an empty run launches nothing: the rows' columns stay as they were)
    same(w.vote_status, g.vote0, "vote0 (the walk's vote_status)", name);
    same(w.pend_take, g.take0, "take0 (the walk's pend_take)", name);
    same(narrowed, g.vote1, "vote1 (all narrowed)", name);
    same(std::vector<uint8_t>(r.att_block.size(), 0), g.take1, "take1 (all zero)", name);
  }
  ++g_walks, g_walks_lag += r.lag, g_walks_early += w.result[kBwStop] < r.n;
}

void check(const Run& r, const char* name) {
  const Out e = reference(r), g = sequential(r);
  if (r.n) {
    same(e.walk, g.walk, "walk", name);
    same(e.base, g.base, "base", name);
  }
  for (int k = 0; k < kBcResultWords; ++k)
    if (e.result[k] != g.result[k]) {
      std::printf("FAIL %s: result[%d] %llu, expected %llu\n", name, k, (unsigned long long)g.result[k], (unsigned long long)e.result[k]);
      std::exit(1);
    }
  same(e.log, g.log, "log", name);
  same(e.ring, g.ring, "ring", name);
  same(e.ring_len, g.ring_len, "ring lengths", name);
  same(e.parents_start, g.parents_start, "parents_start", name);
  same(e.vote0, g.vote0, "vote0", name);
  same(e.vote1, g.vote1, "vote1", name);
  same(e.take0, g.take0, "take0", name);
  same(e.take1, g.take1, "take1", name);
  // the bound of blockcycle_dev.h: no row of a block before stop starts past the entries written for it
  for (size_t i = 0; i < r.att_block.size(); ++i) {
    const uint64_t b = r.att_block[i];
    if (b < e.result[kBwStop] && g.parents_start[i] - r.parents_start[i] + 128 > kBwRing + e.result[kBwNcand]) {
      std::printf("FAIL %s: row %zu of block %llu reads past the log\n", name, i, (unsigned long long)b);
      std::exit(1);
    }
  }
  ++g_runs, g_blocks += r.n, g_rows += r.att_block.size();
  for (uint8_t w : e.walk) g_deferred += w == kBwDeferred, g_saved += w == kBwSaved, g_cands += w == kBwCandidate;
  const bool t = e.result[kBcTIndex] != kBwNone;
  g_with_t += t, g_lag_t += t && r.lag;
  g_l_deferred += t && !r.lag && e.result[kBcLagOut] && e.result[kBwStop] < r.n;
  for (size_t i = 0; i < e.vote1.size(); ++i) g_after += e.vote1[i] == PZ_ATT_PROCESSED || e.take1[i];
  agree_with_walk(r, g, name);
}

void fixed_cases() {
  const uint64_t sizes[] = {0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049};
  const uint64_t far = 1ull << 40;  // a lastStateRecalc no slot below reaches
  for (uint64_t n : sizes) {
    // no T: the walk's runs
    for (int go = 0; go < 3; ++go)
      for (uint64_t lag = 0; lag < 2; ++lag)
        for (uint64_t has0 = 0; has0 < 2; ++has0) {
          check(make(n, go, [](uint64_t j) { return 2 + j; }, has0, 1, far, lag), "increasing");
          check(make(n, go, [](uint64_t j) { return 7 + j / 2; }, has0, 3, far, lag), "siblings");
          check(make(n, go, [n](uint64_t j) { return 2 + n - j; }, has0, 0, far, lag), "decreasing");
          check(make(n, go, [](uint64_t j) { return j % 2; }, has0, 0, far, lag), "slots 0 and 1");
          check(make(n, go, [](uint64_t j) { return (j + 1) % 2; }, has0, 0, far, lag), "slots 1 and 0");
          check(make(n, go, [](uint64_t j) { return j < 3 ? 1 : j; }, has0, 0, far, lag), "ones then up");
          check(make(n, go, [](uint64_t j) { return 2 + j; }, 1, 1ull << 50, far, lag), "a carried candidate above all");
        }
    // T first, in the middle, last, and at both sides of the tile edge (L in the next tile)
    for (uint64_t at : {uint64_t(0), n / 2, n ? n - 1 : 0, uint64_t(1022), uint64_t(1023), uint64_t(1024), uint64_t(2047), uint64_t(2048)}) {
      if (at >= n) continue;
      for (uint64_t has0 = 0; has0 < 2; ++has0) {
        // L right behind T, plain
        check(make(n, 1, [at](uint64_t j) { return j < at ? 10 + j / 40 : 9064 + (j - at); }, has0, 5, 9000, 0), "T, then L");
        check(make(n, 1, [at](uint64_t j) { return j < at ? 10 + j : 9064 + (j - at); }, has0, 5, 9000, 0), "T after candidates, then L");
        // siblings of T and closed blocks between T and L
        check(make(n, 1, [at](uint64_t j) { return j < at ? 10 + j / 40 : j < at + 5 ? 9064 : 9065 + j; }, has0, 5, 9000, 0), "T, siblings, L");
        check(make(n, 2, [at](uint64_t j) { return j < at ? 10 : j < at + 7 ? 9070 - (j - at) : 9071; }, has0, 5, 9000, 0), "T, lower slots and closed blocks, L");
        check(make(n, 3, [at](uint64_t j) { return j < at ? 10 + j / 3 : 9064 + (j - at) / 3; }, has0, 5, 9000, 0), "T, random reports");
        // L a transition itself: a slot jump of a cycle or more
        check(make(n, 1, [at](uint64_t j) { return j < at ? 10 + j : j == at ? 9064 : 9128 + j; }, has0, 5, 9000, 0), "T, then L a transition");
        check(make(n, 1, [at](uint64_t j) { return j < at ? 10 + j : j < at + 3 ? 9064 : 9500 + j; }, has0, 5, 9000, 0), "T, siblings, L a transition");
        // the run ends before an L
        check(make(n, 1, [at](uint64_t j) { return j < at ? 10 + j : 9064; }, has0, 5, 9000, 0), "T, no L");
        // lag 1 with its first candidate at `at`: plain, and a transition
        check(make(n, 1, [at](uint64_t j) { return j < at ? 5 : 6 + j; }, 1, 5, 64, 1), "lag, L plain");
        check(make(n, 1, [at](uint64_t j) { return j < at ? 5 : 128 + j; }, 1, 5, 64, 1), "lag, L a transition");
        check(make(n, 2, [at](uint64_t j) { return j < at ? 5 : 127 + (j - at); }, 1, 5, 64, 1), "lag, alternating");
      }
    }
    check(make(n, 1, [](uint64_t) { return 5; }, 1, 5, far, 1), "lag, no candidate");
    check(make(n, 1, [](uint64_t j) { return 5 + j; }, 0, 0, far, 1), "lag, nothing carried");
    // slots 0 and 1 around a transition that every slot is (last_state_recalc + 64 wraps to 0 and 1)
    check(make(n, 1, [](uint64_t j) { return j % 2; }, 0, 0, ~uint64_t(0) - 63, 0), "slots 0 and 1, all transitions");
    check(make(n, 1, [](uint64_t j) { return j % 2; }, 1, 0, ~uint64_t(0) - 62, 0), "slots 0 and 1, slot 1 a transition");
    check(make(n, 1, [](uint64_t j) { return (j + 1) % 2; }, 0, 0, ~uint64_t(0) - 63, 1), "slots 1 and 0, lag");
    // last_state_recalc near 2^64: both sums wrap
    check(make(n, 1, [](uint64_t j) { return ~uint64_t(0) - 70 + j % 80; }, 0, 0, ~uint64_t(0) - 60, 0), "the sum wraps");
    check(make(n, 1, [](uint64_t j) { return ~uint64_t(0) - 200 + j % 190; }, 0, 0, ~uint64_t(0) - 150, 0), "the second sum wraps");
    check(make(n, 3, [](uint64_t j) { return ~uint64_t(0) - 130 + j % 131; }, 1, 3, ~uint64_t(0) - 127, 1), "lag near 2^64");
  }
}

void random_runs(int count) {
  for (int k = 0; k < count; ++k) {
    const uint64_t n = rng() % 8 == 0 ? rng() % 2200 : rng() % 160;
    const uint64_t lsr = rng() % 6 ? 64 * (rng() % 4) : rng() % 2 ? 1ull << 40 : ~uint64_t(0) - rng() % 200;
    const int shape = (int)(rng() % 5);
    const uint64_t step = 1 + rng() % 3, start = lsr + rng() % 70, jump = rng() % 200;
    auto slot_of = [&](uint64_t j) -> uint64_t {
      switch (shape) {
        case 0: return start + j / step;                 // rising through the cycle's end, with siblings
        case 1: return rng() % (lsr % 1000 + 140);       // anywhere around two cycles
        case 2: return rng() % 3;                        // 0, 1, 2
        case 3: return start + j / step + (j > n / 2 ? jump : 0);  // rising, with a jump
        default: return start + (rng() % 5 ? j / 8 : 0); // rising with drops
      }
    };
    check(make(n, rng() % 3 ? 3 : 1, slot_of, rng() % 2, lsr + rng() % 80, lsr, rng() % 3 == 0), "random");
  }
}

// Runs the walk takes too, at both sides of a wave's and a tile's edge: a last_state_recalc no slot reaches.
void walk_runs() {
  const uint64_t far = 1ull << 40;
  for (uint64_t n : {uint64_t(1), uint64_t(64), uint64_t(65), uint64_t(1023), uint64_t(1024), uint64_t(1025), uint64_t(2049)})
    for (uint64_t lag = 0; lag < 2; ++lag)
      for (int k = 0; k < 8; ++k) {
        const uint64_t at = rng() % (n + 1), step = 1 + rng() % 3;  // under lag: the first candidate, anywhere
        check(make(n, k % 2 ? 3 : 1, [at, step](uint64_t j) { return j < at ? 5 : 6 + j / step; }, 1, 5, far, lag), "the walk's run");
        check(make(n, 3, [](uint64_t) { return rng() % 90; }, rng() % 2, rng() % 90, far, lag), "the walk's run, slots anywhere");
      }
}

}  // namespace

int main() {
  rng.seed(20182);
  fixed_cases();
  random_runs(4000);
  walk_runs();
  std::printf("ok: %llu runs, %llu blocks, %llu deferred, %llu saved-not-candidate, %llu candidates, %llu rows, %llu with T, "
              "%llu with L deferred, %llu with T under lag, %llu rows after T\n",
              (unsigned long long)g_runs, (unsigned long long)g_blocks, (unsigned long long)g_deferred, (unsigned long long)g_saved,
              (unsigned long long)g_cands, (unsigned long long)g_rows, (unsigned long long)g_with_t, (unsigned long long)g_l_deferred,
              (unsigned long long)g_lag_t, (unsigned long long)g_after);
  std::printf("the walk's runs: %llu, %llu under lag, %llu stopped early\n", (unsigned long long)g_walks, (unsigned long long)g_walks_lag,
              (unsigned long long)g_walks_early);
  return 0;
}
