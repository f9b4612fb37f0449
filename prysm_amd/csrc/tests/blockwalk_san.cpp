// The block walk's rules on the CPU under ASan+UBSan: blockwalk_dev.h (the inlines the kernels of
// blockwalk.hip compile too) driven through a sequential form of the scan kernel -- tiles of 1,024
// lanes in waves of 64, the carry between tiles, the two rounds a tile, every lane through the same
// bw_round1 / bw_rank / bw_tile_stop / bw_advance the kernel calls (walk_sequential,
// blockscan_san.h) -- and of the rows, roll and append kernels, against a plain restatement of blockchain/service.go:320-333 that walks block by
// block with a pending-candidate variable and a list that only grows (computeNewActiveState,
// core.go:223-237).  Every array has exactly its size.  Prints counts; exit status 0 iff all agree.
#include "blockscan_san.h"

using namespace san;

namespace {

using Out = WalkOut;

// ---- the reference, block by block ---------------------------------------------------------------
Out reference(const Run& r) {
  Out o;
  o.walk.assign(r.n, kBwDeferred);
  o.base.assign(r.n, 0);
  std::vector<uint8_t> list = r.ring, list_len = r.ring_len;  // a Go slice that is appended to
  bool has = r.has0 != 0;
  uint64_t cslot = has ? r.cslot0 : 0, ncand = 0, stop = r.n;
  for (uint64_t j = 0; j < r.n; ++j) {
    if (r.lag && ncand >= 1) {  // the block after the first candidate: another CrystallizedState
      stop = j;
      break;
    }
    const uint64_t len = list_len.size();
    o.base[j] = len - kBwWindow - r.lag;  // RecentBlockHashes() as this block reads it: the last 128, or with lag the 128 before the last
    if (r.report[j] == 0) {
      o.walk[j] = kBwOff;
      continue;
    }
    const bool had = has;
    if (has && r.slot[j] > cslot && r.slot[j] > 1) has = false;  // updateHead, service.go:320-322
    if (has) {                                                   // :331-333
      o.walk[j] = kBwSaved;
      continue;
    }
    if (r.slot[j] >= r.lsr + 64) {  // IsCycleTransition: the caller's
      has = had, stop = j, o.base[j] = 0;
      break;
    }
    list.insert(list.end(), r.hash.begin() + 32 * j, r.hash.begin() + 32 * j + 32);  // core.go:230-237
    list_len.assign(list_len.size() + 1, 32);  // RecentBlockHashes() is the [32]byte form of every entry, stored back whole
    has = true, cslot = r.slot[j], ++ncand;  // service.go:361
    o.walk[j] = kBwCandidate;
  }
  o.result[kBwStop] = stop, o.result[kBwNcand] = ncand, o.result[kBwHasCandidate] = has, o.result[kBwCandidateSlot] = cslot;
  o.log = list;
  o.log.resize((kBwRing + r.n) * 32, 0);
  o.ring.assign(list.end() - kBwRing * 32, list.end());
  o.ring_len.assign(list_len.end() - kBwRing, list_len.end());
  if (r.flags & 1) o.ring = r.ring, o.ring_len = r.ring_len;  // a panic somewhere in the batch: nothing of it lands
  o.parents_start = r.parents_start, o.pend_take = r.pend_take, o.vote_status = r.vote_status;
  for (size_t i = 0; i < r.att_block.size(); ++i) {
    const uint64_t b = r.att_block[i];
    if (b >= stop) {
      o.pend_take[i] = 0;
      if (o.vote_status[i] == PZ_ATT_PROCESSED) o.vote_status[i] = PZ_ATT_NOT_PROCESSED;
      continue;
    }
    o.parents_start[i] += o.base[b];
    o.pend_take[i] = o.pend_take[i] && o.walk[b] == kBwCandidate;
  }
  return o;
}

uint64_t g_runs, g_blocks, g_deferred, g_saved, g_cands, g_rows, g_appends;

void check(const Run& r, const char* name) {
  const Out e = reference(r), g = walk_sequential(r);
  if (r.n) {
    same(e.walk, g.walk, "walk", name);
    same(e.base, g.base, "base", name);
  }
  for (int k = 0; k < kBwResultWords; ++k)
    if (e.result[k] != g.result[k]) {
      std::printf("FAIL %s: result[%d] %llu, expected %llu\n", name, k, (unsigned long long)g.result[k], (unsigned long long)e.result[k]);
      std::exit(1);
    }
  same(e.log, g.log, "log", name);
  same(e.ring, g.ring, "ring", name);
  same(e.ring_len, g.ring_len, "ring lengths", name);
  same(e.parents_start, g.parents_start, "parents_start", name);
  same(e.pend_take, g.pend_take, "pend_take", name);
  same(e.vote_status, g.vote_status, "vote_status", name);
  ++g_runs, g_blocks += r.n, g_rows += r.att_block.size();
  for (uint8_t w : e.walk) g_deferred += w == kBwDeferred, g_saved += w == kBwSaved, g_cands += w == kBwCandidate;
}

void fixed_cases() {
  const uint64_t sizes[] = {0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049};
  const uint64_t far = 1ull << 40;  // a lastStateRecalc no slot below reaches
  for (uint64_t n : sizes) {
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
    // a transition candidate at 0, in the middle, last, and just past a tile edge
    for (uint64_t at : {uint64_t(0), n / 2, n ? n - 1 : 0, uint64_t(1024), uint64_t(1025), uint64_t(2048)}) {
      if (at >= n) continue;
      for (uint64_t lag = 0; lag < 2; ++lag)
        for (uint64_t has0 = 0; has0 < 2; ++has0) {
          check(make(n, 1, [at](uint64_t j) { return j < at ? 10 + j / 40 : 10000 + j; }, has0, 5, 9000, lag), "transition, siblings before");
          if (!lag) check(make(n, 1, [at](uint64_t j) { return j < at ? 10 + j : 10000 + j; }, has0, 5, 9000, 0), "transition, candidates before");
          check(make(n, 2, [at](uint64_t j) { return j < at ? 10 : 10000 + j; }, has0, 5, 9000, lag), "transition, alternating");
        }
    }
    // lag 1 with the first candidate at 0, at 1024, and absent
    check(make(n, 1, [](uint64_t j) { return 5 + j; }, 0, 0, far, 1), "lag, first candidate at 0");
    check(make(n, 1, [](uint64_t j) { return j < 1024 ? 5 : 6 + j; }, 1, 5, far, 1), "lag, first candidate at 1024");
    check(make(n, 1, [](uint64_t j) { return j < 1023 ? 5 : 6 + j; }, 1, 5, far, 1), "lag, first candidate at 1023");
    check(make(n, 1, [](uint64_t) { return 5; }, 1, 5, far, 1), "lag, no candidate");
    check(make(n, 1, [](uint64_t j) { return ~uint64_t(0) - 70 + j % 80; }, 0, 0, ~uint64_t(0) - 60, 0), "the sum wraps");
  }
}

void random_runs(int count) {
  for (int k = 0; k < count; ++k) {
    const uint64_t n = rng() % 8 == 0 ? rng() % 2200 : rng() % 160;
    const uint64_t lsr = rng() % 4 ? 64 * (rng() % 4) : 1ull << 40;
    const int shape = (int)(rng() % 4);
    const uint64_t step = 1 + rng() % 3, start = rng() % 70;
    auto slot_of = [&](uint64_t j) -> uint64_t {
      switch (shape) {
        case 0: return start + j / step;                 // rising, with siblings
        case 1: return rng() % (lsr % 1000 + 70);        // anywhere around the cycle
        case 2: return rng() % 3;                        // 0, 1, 2
        default: return start + (rng() % 5 ? j / 8 : 0); // rising with drops
      }
    };
    check(make(n, rng() % 3 ? 3 : 1, slot_of, rng() % 2, rng() % 80, lsr, rng() % 4 == 0), "random");
  }
}

// The append: a list model against bw_append_dst over exactly sized arrays.
void appends() {
  for (uint64_t n : {uint64_t(0), uint64_t(1), uint64_t(2), uint64_t(128), uint64_t(129), uint64_t(130), uint64_t(300), uint64_t(1500)})
    for (int mode = 0; mode < 3; ++mode) {  // all, none, random
      std::vector<uint8_t> ring(kBwRing * 32), len(kBwRing), h(32 * n), take(n);
      for (auto& b : ring) b = (uint8_t)rng();
      for (auto& l : len) l = (uint8_t)(rng() % 33);
      for (auto& b : h) b = (uint8_t)rng();
      for (auto& t : take) t = mode == 0 ? 1 : mode == 1 ? 0 : rng() % 2;
      std::vector<uint8_t> list = ring, list_len = len;
      uint64_t total = 0;
      for (uint64_t j = 0; j < n; ++j)
        if (take[j]) list.insert(list.end(), h.begin() + 32 * j, h.begin() + 32 * j + 32), list_len.assign(list_len.size() + 1, 32), ++total;
      std::vector<uint8_t> to(kBwRing * 32, 0xEE), to_len(kBwRing, 0xEE);
      for (uint64_t k = total; k < kBwRing; ++k) std::memcpy(&to[32 * (k - total)], &ring[32 * k], 32), to_len[k - total] = bw_roll_len(len[k], total);
      uint64_t rank = 0;
      for (uint64_t j = 0; j < n; ++j) {
        if (!take[j]) continue;
        const int64_t dst = bw_append_dst(rank++, total);
        if (dst >= 0) std::memcpy(&to[32 * dst], &h[32 * j], 32), to_len[dst] = 32;
      }
      same(std::vector<uint8_t>(list.end() - kBwRing * 32, list.end()), to, "appended ring", "append");
      same(std::vector<uint8_t>(list_len.end() - kBwRing, list_len.end()), to_len, "appended lengths", "append");
      ++g_appends;
    }
}

}  // namespace

int main() {
  rng.seed(20181);
  fixed_cases();
  random_runs(3000);
  appends();
  std::printf("ok: %llu runs, %llu blocks, %llu deferred, %llu saved-not-candidate, %llu candidates, %llu rows, %llu appends\n",
              (unsigned long long)g_runs, (unsigned long long)g_blocks, (unsigned long long)g_deferred, (unsigned long long)g_saved,
              (unsigned long long)g_cands, (unsigned long long)g_rows, (unsigned long long)g_appends);
  return 0;
}
