// The resident transition's pure rules on the CPU, under ASan+UBSan (plain g++; no GPU code):
// votecache_dev.h's vc_probe -- the text pz_vc_lookup_kernel and pz_rs_justify_kernel compile --
// against a std::map over tables and key arrays of exactly their sizes, and recalc_dev.h's
// justification loop, panic decision and clamps against independent restatements.
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "../recalc_dev.h"

using namespace pz;

namespace {

using Key = std::array<uint8_t, 32>;

[[noreturn]] void die(const char* what, long a = 0, long b = 0) {
  std::fprintf(stderr, "FAIL: %s (%ld, %ld)\n", what, a, b);
  std::exit(1);
}

Hash32 as_hash(const Key& k) { return vc_load_hash(k.data()); }

// A key whose home cell in a table of `cells` is `home`, distinct per (tag, salt).
Key key_at(uint32_t home, uint32_t cells, uint32_t tag, uint32_t salt) {
  Key k{};
  const uint32_t w0 = home | (tag * cells);
  std::memcpy(k.data(), &w0, 4);
  std::memcpy(k.data() + 4, &salt, 4);
  for (int i = 8; i < 32; ++i) k[i] = (uint8_t)(tag * 31 + salt * 7 + i);
  return k;
}

// A table and its keys in allocations of exactly their sizes (32-byte aligned, as the device's are):
// one byte past either is ASan's.
struct Table {
  uint32_t cells, nslots = 0, key_room;
  std::vector<uint32_t> table;
  uint8_t* keys;
  std::map<Key, uint32_t> model;
  Table(uint32_t cells_, uint32_t key_room_) : cells(cells_), key_room(key_room_), table(cells_, kVcEmpty) {
    keys = static_cast<uint8_t*>(std::aligned_alloc(32, 32 * (key_room ? key_room : 1)));
  }
  ~Table() { std::free(keys); }
  // the intern and commit launches' end state for one new hash: the first empty cell from home
  void insert(const Key& k) {
    if (nslots >= key_room) die("test: no key room");
    uint32_t c = vc_home(as_hash(k), cells);
    for (uint32_t step = 0; step < cells; ++step, c = vc_next(c, cells))
      if (vc_is_empty(table[c])) {
        std::memcpy(keys + 32ull * nslots, k.data(), 32);
        table[c] = nslots;
        model[k] = nslots++;
        return;
      }
    die("test: table full");
  }
  void check(const Key& k, uint64_t* probes) const {
    const uint32_t got = vc_probe(table.data(), cells, keys, nslots, as_hash(k));
    const auto it = model.find(k);
    const uint32_t want = it == model.end() ? kVcNone : it->second;
    if (got != want) die("probe", got, want);
    ++*probes;
  }
};

uint64_t probe_checks() {
  uint64_t probes = 0;
  for (uint32_t cells : {2u, 4u, 8u})
    for (uint32_t home = 0; home < cells; ++home)       // home == cells - 1: the probe wraps at once
      for (uint32_t fill = 0; fill <= cells; ++fill) {  // fill == cells: a full table
        Table t(cells, cells);
        for (uint32_t k = 0; k < fill; ++k) t.insert(key_at(home, cells, k + 1, 0));
        for (uint32_t k = 0; k < fill; ++k) t.check(key_at(home, cells, k + 1, 0), &probes);  // present
        t.check(key_at(home, cells, 100, 0), &probes);  // absent, the home cell occupied (fill > 0)
        t.check(key_at(home, cells, 1, 9), &probes);    // absent, equal first word, other bytes differ
        t.check(key_at((home + fill) % cells, cells, 101, 0), &probes);  // absent, home empty unless full
      }
  // a claim, and an id the cache never gave out, between the home cell and the key: skipped, never
  // an index (keys holds nslots entries: an index through either is ASan's)
  for (uint32_t odd : {vc_claim(0), vc_claim(5), 0x7FFFFFFFu, 3u}) {
    Table t(8, 3);
    t.insert(key_at(6, 8, 1, 0));  // cell 6, slot 0
    t.table[7] = odd;              // (3 == nslots after the inserts below)
    t.table[0] = odd;
    const Key far = key_at(6, 8, 2, 0);
    std::memcpy(t.keys + 32ull * t.nslots, far.data(), 32);
    t.table[1] = t.nslots;
    t.model[far] = t.nslots++;
    t.insert(key_at(2, 8, 3, 0));
    if (t.nslots != 3) die("test: nslots");
    t.check(far, &probes);
    t.check(key_at(6, 8, 1, 0), &probes);
    t.check(key_at(2, 8, 3, 0), &probes);
    t.check(key_at(6, 8, 50, 0), &probes);  // absent: walks over both odd cells to the empty cell 3
    t.check(key_at(7, 8, 51, 0), &probes);
  }
  // a table of nothing but odd cells: the probe stops after `cells` steps
  for (uint32_t cells : {2u, 8u}) {
    Table t(cells, 0);
    for (uint32_t c = 0; c < cells; ++c) t.table[c] = vc_claim(c);
    t.check(key_at(cells - 1, cells, 1, 0), &probes);
  }
  // random fills of larger tables
  std::mt19937_64 rng(11);
  for (int round = 0; round < 200; ++round) {
    const uint32_t cap = 1 + (uint32_t)(rng() % 40), cells = vc_cells(cap);
    Table t(cells, cap);
    std::vector<Key> ks;
    for (uint32_t k = 0; k < cap; ++k) {
      Key key = key_at((uint32_t)(rng() % cells) % (1 + round % 4), cells, (uint32_t)(rng() % 1000), k);
      ks.push_back(key);
      t.insert(key);
    }
    for (const Key& k : ks) t.check(k, &probes);
    for (uint32_t k = 0; k < cap; ++k) t.check(key_at((uint32_t)(rng() % cells), cells, 2000 + k, k), &probes);
  }
  return probes;
}

// stateRecalc's loop (blockchain/core.go:411-431) restated from the totals, not from a mask, with
// every uint64 operation reduced explicitly.
RsJustified go_loop(const uint64_t totals[64], uint64_t deposits, uint64_t lsr, RsJustified s) {
  typedef unsigned __int128 u128;
  const u128 M = ((u128)1 << 64);
  for (unsigned i = 0; i < 64; ++i) {
    const uint64_t slot = (uint64_t)(((u128)lsr + M - 64 + i) % M);
    const uint64_t lhs = (uint64_t)(((u128)3 * totals[i]) % M), rhs = (uint64_t)(((u128)2 * deposits) % M);
    if (lhs >= rhs) {
      if (slot > s.justified) s.justified = slot;
      s.streak = (uint64_t)(((u128)s.streak + 1) % M);
    } else {
      s.streak = 0;
    }
    const uint64_t back = (uint64_t)(((u128)slot + M - 64) % M);
    if (s.streak >= 65 && back > s.finalized) s.finalized = back;
  }
  return s;
}

uint64_t justify_checks() {
  std::vector<uint64_t> masks = {~0ull, 0ull, 0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull};
  for (int i = 0; i < 64; ++i) masks.push_back(~(1ull << i));
  std::mt19937_64 rng(7);
  for (int i = 0; i < 3000; ++i) masks.push_back(rng() | (i % 3 == 0 ? rng() : 0));
  // totals that pass / fail 3 * bal >= 2 * deposits for deposits in {1, 2^63 + 1} (2 * deposits == 2
  // mod 2^64), some through a triple that wraps
  const uint64_t pass[] = {1, 0x5555555555555556ull, ~0ull, 0x8000000000000000ull};  // triples 3, 2, 2^64 - 3, 2^63
  const uint64_t fail[] = {0, 0xAAAAAAAAAAAAAAABull};                                 // triples 0, 1 (2^65 + 1 wrapped)
  uint64_t n = 0;
  for (uint64_t deposits : {0ull, 1ull, 0x8000000000000001ull})
    for (uint64_t lsr : {0ull, 64ull, 128ull, 0xFFFFFFFFFFFFFFC0ull})
      for (uint64_t streak : {0ull, 1ull, 64ull, ~0ull})
        for (size_t m = 0; m < masks.size(); ++m) {
          if (m >= 68 && (m + streak + lsr / 64) % 4) continue;  // the random masks: a quarter per start
          uint64_t totals[64], mask = 0;
          for (int i = 0; i < 64; ++i) {
            const bool want = (masks[m] >> i) & 1;
            const uint64_t t = want ? pass[(i + m) % 4] : fail[(i + m) % 2];
            totals[i] = t;
            if (rs_slot_passes(t, deposits)) mask |= 1ull << i;
          }
          if (deposits != 0 && mask != masks[m]) die("test: mask not realised", (long)m);
          if (deposits == 0 && mask != ~0ull) die("deposits 0: every slot passes");
          const RsJustified start{streak, lsr / 2, lsr / 4};
          const RsJustified got = rs_justify(mask, lsr, start), want = go_loop(totals, deposits, lsr, start);
          if (got.streak != want.streak || got.justified != want.justified || got.finalized != want.finalized)
            die("justify", (long)m, (long)lsr);
          ++n;
        }
  // the loop's own corners, by hand: 64 passes from a streak of 1 reach 65 at the last slot
  RsJustified r = rs_justify(~0ull, 128, RsJustified{1, 0, 0});
  if (r.streak != 65 || r.justified != 127 || r.finalized != 63) die("hand: streak 1", (long)r.streak, (long)r.finalized);
  r = rs_justify(~0ull, 128, RsJustified{0, 0, 0});
  if (r.streak != 64 || r.justified != 127 || r.finalized != 0) die("hand: streak 0");
  r = rs_justify(~0ull, 0, RsJustified{64, 5, 7});  // slots 2^64 - 64 ..: justified and finalized jump
  if (r.streak != 128 || r.justified != ~0ull || r.finalized != ~0ull - 64) die("hand: wrap");
  r = rs_justify(0, 128, RsJustified{~0ull, 3, 2});
  if (r.streak != 0 || r.justified != 3 || r.finalized != 2) die("hand: all fail");
  r = rs_justify(~0ull, 64, RsJustified{~0ull, 0, 0});  // the streak wraps to 0 at the first slot
  if (r.streak != 63 || r.finalized != 0) die("hand: streak wraps");
  return n + 5;
}

uint64_t commit_checks() {
  uint64_t n = 0;
  // the panic decision against a restatement in Python's shape (blockchain.state_recalc_device)
  std::mt19937_64 rng(3);
  const uint64_t pops[] = {0, 1, 21, 22, 1ull << 40, 0x0155555555555555ull, 0x0155555555555556ull, ~0ull};
  const uint64_t deps[] = {0, 1, 1024, 32768, 0x8000000000000001ull, ~0ull};
  for (uint64_t pop : pops)
    for (uint64_t dep : deps)
      for (uint64_t nact : {0ull, 1ull, 4096ull})
        for (uint64_t xl : {0ull, 1ull, 4ull, 12ull})
          for (uint64_t rwd : {0ull, 1ull, 7ull}) {
            uint64_t scal[PZ_SCAL_COUNT];
            for (auto& x : scal) x = rng();
            scal[PZ_SCAL_POP] = pop, scal[PZ_SCAL_NACT] = nact, scal[PZ_SCAL_ERR_XL] = xl, scal[PZ_SCAL_ERR_RWD] = rwd;
            typedef unsigned __int128 u128;
            const uint64_t lhs = (uint64_t)((u128)pop * 96), rhs = (uint64_t)((u128)dep * 2);
            const bool want = xl != 0 || (lhs >= rhs && nact > 0 && rwd != 0);
            if (rs_panics(scal, dep) != want) die("panics", (long)pop, (long)dep);
            ++n;
          }
  // the clamps
  for (uint32_t stride : {32u, 48u, 256u}) {
    if (!rs_stride_ok(stride)) die("stride ok", stride);
    for (uint64_t lo : {0ull, 5ull, 1ull << 40})
      for (uint64_t len = 0; len <= stride + 40ull; ++len) {
        const uint32_t got = rs_hash_len(lo, lo + len, stride);
        if (got != (len > stride ? stride : len)) die("hash_len", (long)len, stride);
        if (rs_row_fits(lo, lo + len, stride) != (len <= stride)) die("row_fits", (long)len, stride);
        ++n;
      }
    if (rs_hash_len(10, 3, stride) != 0 || !rs_row_fits(10, 3, stride)) die("inverted range");
    if (rs_hash_len(0, ~0ull, stride) != stride || rs_row_fits(0, ~0ull, stride)) die("huge range");
  }
  for (uint32_t stride : {0u, 16u, 31u, 33u, 40u, 257u, 272u, 0xFFFFFFF0u})
    if (rs_stride_ok(stride)) die("stride refused", stride);
  if (rs_row_ok(kRsNoWinner, ~0ull) || rs_row_ok(5, 5) || rs_row_ok(0, 0) || !rs_row_ok(4, 5) || !rs_row_ok(0, 1)) die("row_ok");
  // copying by the clamp never leaves the row: a record buffer and a pool column of exact sizes
  for (uint32_t stride : {32u, 64u})
    for (uint64_t len : {0ull, 1ull, 31ull, 32ull, 33ull, 64ull, 65ull, 300ull}) {
      std::vector<uint8_t> col(7 + len), rec(stride, 0xEE);
      for (uint64_t k = 0; k < col.size(); ++k) col[k] = (uint8_t)(k * 13 + 1);
      const uint32_t take = rs_hash_len(7, 7 + len, stride);
      std::memset(rec.data(), 0, stride);
      std::memcpy(rec.data(), col.data() + 7, take);
      if (take && rec[take - 1] != col[7 + take - 1]) die("copy", (long)len);
      ++n;
    }
  return n + 20;
}

}  // namespace

int main() {
  const uint64_t probes = probe_checks();
  const uint64_t masks = justify_checks();
  const uint64_t commits = commit_checks();
  std::printf("ok: %llu probes, %llu masks, %llu commit decisions\n", (unsigned long long)probes, (unsigned long long)masks,
              (unsigned long long)commits);
  return 0;
}
