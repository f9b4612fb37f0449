// The vote cache's growth and retirement rules (votecache_dev.h: vc_keep_mark, vc_kept, vc_new_id,
// vc_rehash_insert, vc_row_head) on the CPU under ASan+UBSan: a sequential, lane-by-lane form of the
// keep, renumber, move and rehash launches of votecache.hip over the header's own inlines, against
// a std::map model filtered by the keep list.  The destination buffer set starts full of stale
// bytes, as after an earlier swap, and every array has exactly its size, so ASan guards both ends
// of every row.  The rehash visits the slots in a shuffled order (the schedule the device does not
// promise).  Covers: keep none and keep all, duplicate and absent keep-hashes, the all-zero key,
// keys whose home cell is the last cell (the probe wraps), nslots of 0, 1, one tile and one tile
// + 1, rows of 1..9 words (every head and tail), and the reserve (every slot keeps its id).
// No GPU code involved.
//   g++ -fsanitize=address,undefined tests/votecache_retain_san.cpp && ./a.out
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../votecache_dev.h"

using namespace pz;
using Key = std::array<uint8_t, 32>;

#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                            \
    }                                                          \
  } while (0)

constexpr uint32_t kTile = 256;  // the renumber launch's tile (tile_scan.h)

struct Entry {
  uint64_t total;
  std::vector<uint32_t> voters;
};

// One buffer set, every array at exactly its size.
struct Set {
  uint32_t slot_cap, cells;
  uint64_t words;
  std::vector<uint32_t> bitmaps, table;
  std::vector<uint64_t> totals;
  std::vector<uint8_t> keys;
  Set(uint32_t cap, uint64_t w, uint8_t fill)
      : slot_cap(cap), cells(vc_cells(cap)), words(w), bitmaps(cap * w, 0x01010101u * fill), table(cells, fill ? 0x5A5A5A5Au : kVcEmpty),
        totals(cap, fill ? 0xABABABABABABABABull : 0), keys(32ull * cap, fill) {}
};

static Hash32 hash_of(const Key& k) { return vc_load_hash(k.data()); }

static bool claim_seq(std::vector<uint32_t>& table, uint32_t c, uint32_t slot) {
  if (table[c] != kVcEmpty) return false;
  table[c] = slot;
  return true;
}

// A cache of n distinct keys in slot order, as tallies leave it (the table through the same probe).
static void fill(Set& s, const std::vector<Key>& keys, std::map<Key, Entry>& model, std::mt19937_64& rng) {
  for (uint32_t slot = 0; slot < keys.size(); ++slot) {
    std::memcpy(s.keys.data() + 32ull * slot, keys[slot].data(), 32);
    Entry e;
    e.total = rng();
    e.voters.resize(s.words);
    for (auto& w : e.voters) w = (uint32_t)rng();
    s.totals[slot] = e.total;
    std::copy(e.voters.begin(), e.voters.end(), s.bitmaps.begin() + slot * s.words);
    model[keys[slot]] = e;
    CHECK(vc_rehash_insert(s.cells, hash_of(keys[slot]), [&](uint32_t c) { return claim_seq(s.table, c, slot); }) != kVcNone);
  }
}

// The launches, lane by lane.  retain: keep | renumber | move | rehash; else (a reserve) move | rehash.
static uint32_t run_move(const Set& from, uint32_t nslots, Set& to, bool retain, const std::vector<uint8_t>& hashes, uint64_t n,
                         std::vector<uint32_t>* new_id_out, std::mt19937_64& rng) {
  std::vector<uint32_t> flag(from.slot_cap, 0), new_id(from.slot_cap, 0xDEADBEEFu), old_of(from.slot_cap, 0xDEADBEEFu);
  uint32_t count = nslots;
  if (retain) {
    for (uint64_t q = 0; q < n; ++q) {  // keep: a lane per keep-hash
      // (a 16-byte aligned copy: vc_load_hash16 asks for it, as the device form does)
      alignas(16) uint8_t row[32];
      std::memcpy(row, hashes.data() + 32 * q, 32);
      const uint32_t slot = vc_keep_mark(from.table.data(), from.cells, from.keys.data(), nslots, vc_load_hash16(row));
      if (slot != kVcNone) {
        CHECK(slot < nslots);
        flag[slot] = 1;
      }
    }
    uint64_t kept_before = 0;  // renumber: a tile at a time, each lane its exclusive count within the tile
    for (uint64_t s0 = 0; s0 < nslots; s0 += kTile) {
      uint64_t in_tile = 0;
      for (uint32_t lane = 0; lane < kTile; ++lane) {
        const uint64_t s = s0 + lane;
        const bool kept = vc_kept(flag.data(), nslots, s);
        const uint32_t id = vc_new_id(kept, kept_before + in_tile);
        if (s < nslots) new_id[s] = id;
        if (kept) {
          CHECK(id < from.slot_cap);
          old_of[id] = (uint32_t)s;
          ++in_tile;
        }
      }
      kept_before += in_tile;
    }
    count = (uint32_t)kept_before;
  }
  // move: per_row lanes a destination row, every row of the new set
  const uint64_t w = from.words, per_row = w / 4 + 1;
  for (uint64_t d = 0; d < to.slot_cap; ++d) {
    const bool live = d < count;
    const uint64_t o = live ? (retain ? old_of[d] : d) : 0;
    if (live) CHECK(o < from.slot_cap);
    const uint32_t head = vc_row_head(d * w, w);
    const uint64_t pieces = (w - head) / 4;
    CHECK(pieces < per_row);
    CHECK(head == w || ((d * w + head) & 3) == 0);  // the pieces' stores are 16-byte aligned
    for (uint64_t i = 0; i < per_row; ++i) {
      if (i < pieces) {
        uint32_t v[4] = {0, 0, 0, 0};
        if (live) std::memcpy(v, from.bitmaps.data() + o * w + head + 4 * i, 16);
        std::memcpy(to.bitmaps.data() + d * w + head + 4 * i, v, 16);
      }
      if (i != 0) continue;
      for (uint64_t k = 0; k < head; ++k) to.bitmaps[d * w + k] = live ? from.bitmaps[o * w + k] : 0;
      for (uint64_t k = head + 4 * pieces; k < w; ++k) to.bitmaps[d * w + k] = live ? from.bitmaps[o * w + k] : 0;
      to.totals[d] = live ? from.totals[o] : 0;
      if (live) std::memcpy(to.keys.data() + 32 * d, from.keys.data() + 32 * o, 32);
      else std::memset(to.keys.data() + 32 * d, 0, 32);
    }
  }
  // rehash: the table cleared, then a lane per new slot, in any order
  std::fill(to.table.begin(), to.table.end(), kVcEmpty);
  std::vector<uint32_t> order(count);
  for (uint32_t s = 0; s < count; ++s) order[s] = s;
  std::shuffle(order.begin(), order.end(), rng);
  for (uint32_t s : order)
    CHECK(vc_rehash_insert(to.cells, vc_load_hash16(to.keys.data() + 32ull * s), [&](uint32_t c) { return claim_seq(to.table, c, s); }) != kVcNone);
  if (new_id_out) *new_id_out = new_id;
  return count;
}

// The new set against the model filtered by `keep` (NULL: everything, a reserve).
static void check(const Set& to, uint32_t count, const std::vector<Key>& old_keys, const std::map<Key, Entry>& model,
                  const std::set<Key>* keep) {
  std::vector<Key> want;  // ascending old id
  for (const Key& k : old_keys)
    if (!keep || keep->count(k)) want.push_back(k);
  CHECK(count == want.size());
  for (uint32_t s = 0; s < count; ++s) {
    const Entry& e = model.at(want[s]);
    CHECK(!std::memcmp(to.keys.data() + 32ull * s, want[s].data(), 32));
    CHECK(to.totals[s] == e.total);
    CHECK(std::equal(e.voters.begin(), e.voters.end(), to.bitmaps.begin() + s * to.words));
    CHECK(vc_probe(to.table.data(), to.cells, to.keys.data(), count, hash_of(want[s])) == s);
  }
  for (uint64_t s = count; s < to.slot_cap; ++s) {  // fresh slots read zero, whatever the set held
    CHECK(to.totals[s] == 0);
    for (uint64_t k = 0; k < to.words; ++k) CHECK(to.bitmaps[s * to.words + k] == 0);
  }
  for (const Key& k : old_keys)
    if (keep && !keep->count(k)) CHECK(vc_probe(to.table.data(), to.cells, to.keys.data(), count, hash_of(k)) == kVcNone);
  std::vector<uint32_t> seen(count, 0);  // every cell empty or one slot's, every slot in one cell
  for (uint32_t v : to.table)
    if (v != kVcEmpty) {
      CHECK(v < count);
      ++seen[v];
    }
  for (uint32_t s = 0; s < count; ++s) CHECK(seen[s] == 1);
}

static Key random_key(std::mt19937_64& rng) {
  Key k;
  for (auto& b : k) b = (uint8_t)rng();
  return k;
}

// n distinct keys for a cache of `cap` slots: the all-zero key, `last` keys whose home cell is the
// table's last cell, random ones.
static std::vector<Key> make_keys(uint32_t n, uint32_t cap, bool zero, uint32_t last, std::mt19937_64& rng) {
  std::set<Key> have;
  std::vector<Key> keys;
  const uint32_t cells = vc_cells(cap);
  while (keys.size() < n) {
    Key k = random_key(rng);
    if (zero && keys.empty()) k.fill(0);
    else if (keys.size() <= last) {
      const uint32_t w0 = ((uint32_t)rng() & ~(cells - 1)) | (cells - 1);
      for (int j = 0; j < 4; ++j) k[j] = (uint8_t)(w0 >> (8 * j));
      CHECK(vc_home(hash_of(k), cells) == cells - 1);
    }
    if (have.insert(k).second) keys.push_back(k);
  }
  std::shuffle(keys.begin(), keys.end(), rng);
  return keys;
}

enum Mode { kNone, kAll, kRandom };

static void one_case(uint32_t nslots, uint32_t cap, uint64_t words, Mode mode, bool zero, uint32_t last, std::mt19937_64& rng) {
  Set from(cap, words, 0);
  std::map<Key, Entry> model;
  const std::vector<Key> keys = make_keys(nslots, cap, zero, last, rng);
  fill(from, keys, model, rng);
  // the keep list: chosen keys, some twice, and hashes the map lacks (some sharing a kept key's home cell)
  std::set<Key> keep;
  std::vector<Key> list;
  for (const Key& k : keys)
    if (mode == kAll || (mode == kRandom && (rng() & 1))) {
      keep.insert(k);
      list.push_back(k);
      if (rng() % 4 == 0) list.push_back(k);
    }
  if (mode != kNone)
    for (int j = 0; j < 5; ++j) {
      Key k = random_key(rng);
      if (j & 1 && !keys.empty()) std::memcpy(k.data(), keys[rng() % keys.size()].data(), 4);
      if (!model.count(k)) list.push_back(k);
    }
  std::shuffle(list.begin(), list.end(), rng);
  std::vector<uint8_t> hashes(32 * list.size());  // (exactly n x 32 bytes)
  for (size_t q = 0; q < list.size(); ++q) std::memcpy(hashes.data() + 32 * q, list[q].data(), 32);

  Set kept(cap, words, 0xAB);  // a stale other set
  std::vector<uint32_t> new_id;
  const uint32_t count = run_move(from, nslots, kept, true, hashes, list.size(), &new_id, rng);
  check(kept, count, keys, model, &keep);
  uint32_t rank = 0;
  for (uint32_t s = 0; s < nslots; ++s) CHECK(new_id[s] == (keep.count(keys[s]) ? rank++ : kVcDropped));

  // a second retain in a row reaches the first set again, stale now: keep every other kept key
  std::vector<Key> kept_keys;
  for (const Key& k : keys)
    if (keep.count(k)) kept_keys.push_back(k);
  std::set<Key> keep2;
  std::vector<uint8_t> hashes2;
  for (size_t j = 0; j < kept_keys.size(); j += 2) {
    keep2.insert(kept_keys[j]);
    hashes2.insert(hashes2.end(), kept_keys[j].begin(), kept_keys[j].end());
  }
  const uint32_t count2 = run_move(kept, count, from, true, hashes2, keep2.size(), nullptr, rng);
  check(from, count2, kept_keys, model, &keep2);

  // a reserve from there: more slots, another cell count, every entry where it was
  std::vector<Key> last_keys;
  for (const Key& k : kept_keys)
    if (keep2.count(k)) last_keys.push_back(k);
  Set grown(cap + 1 + (uint32_t)(rng() % (2 * cap + 1)), words, 0xCD);
  const uint32_t count3 = run_move(from, count2, grown, false, {}, 0, nullptr, rng);
  check(grown, count3, last_keys, model, nullptr);
}

int main() {
  std::mt19937_64 rng(20181031);
  CHECK(vc_row_head(0, 5) == 0 && vc_row_head(1, 5) == 3 && vc_row_head(2, 5) == 2 && vc_row_head(3, 5) == 1);
  CHECK(vc_row_head(3, 1) == 1 && vc_row_head(1, 2) == 2 && vc_row_head(4, 0) == 0);
  int cases = 0;
  const uint32_t sizes[] = {0, 1, 2, 7, kTile - 1, kTile, kTile + 1, 2 * kTile + 3};
  for (uint32_t nslots : sizes)
    for (uint64_t words = 1; words <= 9; ++words)
      for (Mode mode : {kNone, kAll, kRandom})
        for (int rep = 0; rep < 2; ++rep) {
          const uint32_t cap = std::max<uint32_t>(1, nslots + (rep ? (uint32_t)(rng() % 9) : 0));  // rep 0: a full cache
          one_case(nslots, cap, words, mode, /*zero=*/(rep & 1) != 0 || nslots == 1, /*last=*/std::min<uint32_t>(nslots, 4), rng);
          ++cases;
        }
  for (int rep = 0; rep < 300; ++rep) {  // small tables: long probes, every wrap
    const uint32_t cap = 1 + (uint32_t)(rng() % 12), nslots = (uint32_t)(rng() % (cap + 1));
    one_case(nslots, cap, 1 + rng() % 6, kRandom, rng() & 1, nslots, rng);
    ++cases;
  }
  std::printf("ok: %d caches retained twice and reserved\n", cases);
  return 0;
}
