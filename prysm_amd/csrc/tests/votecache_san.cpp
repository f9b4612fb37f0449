// The vote cache's table rules (votecache_dev.h) on the CPU under ASan+UBSan: a sequential form
// of phases 1-3 of votecache.hip (mark, intern, commit) over the header's own inlines, against a
// std::map model written from blockchain/core.go:300-360 with byte vectors.  The intern phase
// visits the used sources in a shuffled order (the schedule the device does not promise), so the
// claims, their lowering to the smallest source index and the deterministic slot numbering are
// all exercised.  Covers random batches, tables of 2-8 cells in which every hash shares one home
// cell, and the rollback of a call that does not fit.  No GPU code involved.
//   g++ -fsanitize=address,undefined tests/votecache_san.cpp && ./a.out
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../votecache_dev.h"

using namespace pz;
using Bytes = std::vector<uint8_t>;
using Key = std::array<uint8_t, 32>;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);          \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

struct Batch {
  uint64_t natt = 0, n_recent = 0;
  Bytes recent;                       // n_recent x 32
  Bytes obl;                          // the elements' bytes, exactly (ASan guards both ends)
  std::vector<uint64_t> ooffs, first, pstart;
  std::vector<uint8_t> live;          // status PROCESSED and taken
  uint64_t nsrc() const { return n_recent + (ooffs.size() - 1); }
};

struct Cache {
  uint32_t slot_cap, cells, nslots = 0;
  std::vector<uint32_t> table;
  std::vector<Key> keys;
  uint64_t err = 0;
  explicit Cache(uint32_t cap) : slot_cap(cap), cells(vc_cells(cap)), table(cells, kVcEmpty), keys(cap) {}
};

struct CallOut {
  std::vector<uint64_t> mask;
  std::vector<uint32_t> src_slot;
  bool is_void = false;
};

static Key key_of(const Hash32& h) {
  Key k;
  for (int j = 0; j < 32; ++j) k[j] = (uint8_t)(h.w[j >> 2] >> (8 * (j & 3)));
  return k;
}

static Hash32 source_hash(const Batch& b, uint64_t s) {
  if (s < b.n_recent) return vc_load_hash(b.recent.data() + 32 * s);
  const uint64_t e = s - b.n_recent;
  return vc_bytes_to_hash(b.obl.data(), b.ooffs[e], b.ooffs[e + 1]);
}

// ---- the sequential form of the kernels -----------------------------------------------------
static CallOut run_call(Cache& c, const Batch& b, std::mt19937_64& rng) {
  const uint64_t nsrc = b.nsrc();
  CallOut o;
  o.mask.assign(b.natt, 0);
  o.src_slot.assign(nsrc, kVcNone);
  std::vector<uint8_t> used(nsrc, 0);
  std::vector<uint32_t> src_cell(nsrc, kVcNone);
  // 1: mark
  for (uint64_t i = 0; i < b.natt; ++i) {
    const uint64_t f0 = b.first[i], m = b.first[i + 1] - f0, ps = b.pstart[i];
    if (!b.live[i] || !vc_parents_in_range(m, ps, b.n_recent)) continue;
    Hash32 h[kVcParents];
    uint64_t len[kVcParents];
    for (uint32_t r = 0; r < kVcParents; ++r) {
      const uint64_t s = vc_parent_source(r, m, ps, f0, b.n_recent);
      h[r] = source_hash(b, s);
      len[r] = s < b.n_recent ? 0 : b.ooffs[s - b.n_recent + 1] - b.ooffs[s - b.n_recent];
    }
    for (uint32_t r = 0; r < kVcParents; ++r) {
      bool skip = false;
      for (uint32_t q = 0; q < kVcParents; ++q) skip = skip || vc_skipped_by(h[r], h[q], len[q]);
      if (skip) continue;
      used[vc_parent_source(r, m, ps, f0, b.n_recent)] = 1;
      o.mask[i] |= 1ull << r;
    }
  }
  // 2: intern, in a shuffled order
  std::vector<uint64_t> order;
  for (uint64_t s = 0; s < nsrc; ++s)
    if (used[s]) order.push_back(s);
  std::shuffle(order.begin(), order.end(), rng);
  bool overflow = false;
  for (uint64_t s : order) {
    const Hash32 h = source_hash(b, s);
    const uint32_t mine = vc_claim((uint32_t)s);
    uint32_t cell = vc_home(h, c.cells);
    bool done = false;
    for (uint32_t step = 0; step < c.cells && !done; ++step, cell = vc_next(cell, c.cells)) {
      CHECK(cell < c.cells);
      uint32_t v = c.table[cell];
      if (vc_is_empty(v)) {
        c.table[cell] = mine;  // (the CAS, alone on the table)
        src_cell[s] = cell;
        done = true;
      } else if (vc_is_slot(v)) {
        CHECK(v < c.nslots);
        if (key_of(h) == c.keys[v]) {
          o.src_slot[s] = v;
          done = true;
        }
      } else {
        CHECK(vc_is_claim(v));
        const uint32_t t = vc_claim_source(v);
        CHECK(t < nsrc);
        if (vc_hash_eq(h, source_hash(b, t))) {
          c.table[cell] = std::min(v, mine);
          src_cell[s] = cell;
          done = true;
        }
      }
      if (done) break;
    }
    if (!done) overflow = true;
  }
  // 3: commit
  auto leads = [&](uint64_t s) { return used[s] && src_cell[s] != kVcNone && c.table[src_cell[s]] == vc_claim((uint32_t)s); };
  uint64_t fresh = 0;
  for (uint64_t s = 0; s < nsrc; ++s)
    if (leads(s)) o.src_slot[s] = (uint32_t)(c.nslots + fresh++);
  if (overflow || c.nslots + fresh > c.slot_cap) {
    for (uint64_t s = 0; s < nsrc; ++s)
      if (leads(s)) c.table[src_cell[s]] = kVcEmpty;
    c.err |= kVcErrCapacity;
    o.is_void = true;
    return o;
  }
  for (uint64_t s = 0; s < nsrc; ++s) {
    if (!used[s] || src_cell[s] == kVcNone) continue;
    const uint32_t t = vc_claim_source(c.table[src_cell[s]]);
    if (t == s) c.keys[o.src_slot[s]] = key_of(source_hash(b, s));
    else o.src_slot[s] = o.src_slot[t];
  }
  for (uint64_t s = 0; s < nsrc; ++s)
    if (leads(s)) c.table[src_cell[s]] = o.src_slot[s];
  c.nslots += (uint32_t)fresh;
  return o;
}

// ---- the model: Go's loop over byte vectors ---------------------------------------------------
static Key bytes_to_hash(const uint8_t* p, uint64_t n) {  // common.BytesToHash
  Key k{};
  if (n > 32) p += n - 32, n = 32;
  std::copy(p, p + n, k.begin() + (32 - n));
  return k;
}

struct Model {
  std::map<Key, uint32_t> slot;
  std::vector<Key> keys;
};

// The (attestation, r) -> hash list Go tallies, and the new hashes with their smallest source.
static bool model_call(Model& M, uint32_t slot_cap, const Batch& b, std::vector<std::vector<std::pair<uint32_t, Key>>>* tallied) {
  std::map<Key, uint64_t> fresh;
  tallied->assign(b.natt, {});
  for (uint64_t i = 0; i < b.natt; ++i) {
    const uint64_t f0 = b.first[i], m = b.first[i + 1] - f0, ps = b.pstart[i];
    if (!b.live[i] || m > 64 || ps + 64 - m > b.n_recent) continue;
    std::vector<Bytes> raw;
    for (uint64_t e = f0; e < f0 + m; ++e) raw.emplace_back(b.obl.begin() + b.ooffs[e], b.obl.begin() + b.ooffs[e + 1]);
    for (uint32_t r = 0; r < 64; ++r) {
      Key h;
      uint64_t src;
      if (r < 64 - m) {
        src = ps + r;
        std::copy(b.recent.begin() + 32 * src, b.recent.begin() + 32 * src + 32, h.begin());
      } else {
        const Bytes& e = raw[r - (64 - m)];
        src = b.n_recent + f0 + (r - (64 - m));
        h = bytes_to_hash(e.data(), e.size());
      }
      bool skip = false;
      for (const Bytes& e : raw) skip = skip || (e.size() == 32 && std::equal(e.begin(), e.end(), h.begin()));
      if (skip) continue;
      (*tallied)[i].push_back({r, h});
      if (!M.slot.count(h)) {
        auto it = fresh.find(h);
        if (it == fresh.end()) fresh[h] = src;
        else it->second = std::min(it->second, src);
      }
    }
  }
  if (M.keys.size() + fresh.size() > slot_cap) return false;
  std::vector<std::pair<uint64_t, Key>> ord;
  for (auto& kv : fresh) ord.push_back({kv.second, kv.first});
  std::sort(ord.begin(), ord.end());
  for (auto& sk : ord) {
    M.slot[sk.second] = (uint32_t)M.keys.size();
    M.keys.push_back(sk.second);
  }
  return true;
}

// Every key is found again from its home cell, and nothing else is in the table.
static void check_table(const Cache& c, const Model& M) {
  CHECK(c.nslots == M.keys.size());
  uint32_t occupied = 0;
  for (uint32_t v : c.table) {
    CHECK(vc_is_empty(v) || (vc_is_slot(v) && v < c.nslots));
    occupied += !vc_is_empty(v);
  }
  CHECK(occupied == c.nslots);
  for (uint32_t s = 0; s < c.nslots; ++s) {
    CHECK(c.keys[s] == M.keys[s]);
    Hash32 h = vc_load_hash(c.keys[s].data());
    uint32_t cell = vc_home(h, c.cells), step = 0;
    for (; step < c.cells; ++step, cell = vc_next(cell, c.cells)) {
      CHECK(!vc_is_empty(c.table[cell]));  // an empty cell before the key would hide it
      if (c.table[cell] == s) break;
    }
    CHECK(step < c.cells);
  }
}

static Batch random_batch(std::mt19937_64& rng, uint64_t natt, uint64_t n_recent, const std::vector<Key>& pool, int max_m) {
  Batch b;
  b.natt = natt;
  b.n_recent = n_recent;
  auto pick = [&]() { return pool[rng() % pool.size()]; };
  for (uint64_t k = 0; k < n_recent; ++k) {
    const Key h = pick();
    b.recent.insert(b.recent.end(), h.begin(), h.end());
  }
  static const int kLens[] = {0, 1, 31, 32, 32, 33, 40};
  b.ooffs.push_back(0);
  b.first.push_back(0);
  for (uint64_t i = 0; i < natt; ++i) {
    const uint64_t m = max_m ? rng() % (max_m + 1) : 0;
    for (uint64_t e = 0; e < m; ++e) {
      const int len = kLens[rng() % 7];
      const Key h = pick();  // its tail is a pool hash: elements collide with recent entries
      Bytes el(len);
      for (int j = 0; j < len; ++j) el[len - 1 - j] = j < 32 ? h[31 - j] : (uint8_t)rng();
      b.obl.insert(b.obl.end(), el.begin(), el.end());
      b.ooffs.push_back(b.obl.size());
    }
    b.first.push_back(b.ooffs.size() - 1);
    const uint64_t room = n_recent >= 64 - m ? n_recent - (64 - m) : 0;
    b.pstart.push_back(rng() % 8 == 0 ? n_recent : rng() % (room + 1));  // (some rows out of range)
    b.live.push_back(rng() % 5 != 0);
  }
  return b;
}

static std::vector<Key> make_pool(std::mt19937_64& rng, size_t n, bool colliding) {
  std::vector<Key> pool(n);
  for (size_t k = 0; k < n; ++k) {
    for (auto& x : pool[k]) x = (uint8_t)rng();
    if (colliding) pool[k][0] = 0xFF, pool[k][1] = 0xFF, pool[k][2] = 0xFF, pool[k][3] = 0xFF;  // home = the last cell
    if (k % 7 == 3) std::fill(pool[k].begin(), pool[k].begin() + 20, 0);  // short-looking hashes
  }
  return pool;
}

static void scenario(std::mt19937_64& rng, uint32_t slot_cap, size_t pool_n, bool colliding, int calls, uint64_t natt,
                     uint64_t n_recent, int max_m, int* landed, int* dropped) {
  const std::vector<Key> pool = make_pool(rng, pool_n, colliding);
  Cache c(slot_cap);
  Model M;
  for (int call = 0; call < calls; ++call) {
    const Batch b = random_batch(rng, natt, n_recent, pool, max_m);
    const Cache before = c;
    std::vector<std::vector<std::pair<uint32_t, Key>>> tallied;
    const bool fits = model_call(M, slot_cap, b, &tallied);
    const CallOut o = run_call(c, b, rng);
    CHECK(o.is_void == !fits);
    if (!fits) {  // the rollback: the table, the keys and nslots are what they were
      CHECK(c.table == before.table && c.keys == before.keys && c.nslots == before.nslots);
      CHECK(c.err & kVcErrCapacity);
      ++*dropped;
    } else {
      ++*landed;
      for (uint64_t i = 0; i < b.natt; ++i) {
        uint64_t want = 0;
        for (auto& rk : tallied[i]) {
          want |= 1ull << rk.first;
          const uint64_t m = b.first[i + 1] - b.first[i];
          const uint64_t s = vc_parent_source(rk.first, m, b.pstart[i], b.first[i], b.n_recent);
          CHECK(o.src_slot[s] == M.slot.at(rk.second));
        }
        CHECK(o.mask[i] == want);
      }
    }
    check_table(c, M);
  }
}

int main() {
  std::mt19937_64 rng(20240607);
  CHECK(vc_cells(1) == 2 && vc_cells(2) == 4 && vc_cells(3) == 8 && vc_cells(4) == 8 && vc_cells(5) == 16);
  CHECK(vc_cells(kVcMaxSlotCap) == 0x80000000u);
  CHECK(vc_is_empty(kVcEmpty) && !vc_is_claim(kVcEmpty) && !vc_is_slot(kVcEmpty));
  CHECK(vc_is_claim(vc_claim(0)) && vc_claim_source(vc_claim(0x7FFFFFFE)) == 0x7FFFFFFE && !vc_is_empty(vc_claim(0x7FFFFFFE)));
  // BytesToHash from a range, every length 0..70 at every start 0..3, in an exact-size buffer
  for (uint64_t len = 0; len <= 70; ++len)
    for (uint64_t lo = 0; lo < 4; ++lo) {
      Bytes buf(lo + len);
      for (auto& x : buf) x = (uint8_t)rng();
      CHECK(key_of(vc_bytes_to_hash(buf.data(), lo, lo + len)) == bytes_to_hash(buf.data() + lo, len));
    }
  int landed = 0, dropped = 0;
  // random batches, a roomy table
  for (int k = 0; k < 20; ++k) scenario(rng, 2048, 150, false, 4, 24, 128, 5, &landed, &dropped);
  for (int k = 0; k < 5; ++k) scenario(rng, 4096, 300, false, 3, 12, 100, 64, &landed, &dropped);
  CHECK(dropped == 0);
  // 2-8 cells, every hash with the same home cell (the last one: the probe wraps)
  for (uint32_t cap = 1; cap <= 4; ++cap)
    for (int k = 0; k < 40; ++k) scenario(rng, cap, cap, true, 3, 3, 64, 2, &landed, &dropped);
  // the rollback: more distinct hashes than slots
  const int before = dropped;
  for (uint32_t cap = 1; cap <= 4; ++cap)
    for (int k = 0; k < 40; ++k) scenario(rng, cap, cap + 2, true, 6, 2, 64, 2, &landed, &dropped);
  for (int k = 0; k < 10; ++k) scenario(rng, 40, 60, false, 6, 6, 80, 3, &landed, &dropped);
  CHECK(dropped > before && landed > 100);
  std::printf("ok: %d calls landed, %d rolled back\n", landed, dropped);
  return 0;
}
