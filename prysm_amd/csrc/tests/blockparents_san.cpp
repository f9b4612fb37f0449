// The parent check's rules and the saved-block set's table on the CPU under ASan+UBSan:
// blockparents_dev.h (the inlines the kernels of blockparents.hip compile too) driven through a
// sequential form of the three launches of pz_dev_block_parents (open, link, and the double-buffered
// pointer-jumping rounds), of the insert (tiles of 1,024 lanes taken in a shuffled order, so that a
// lane of lower index meets a higher one's claim), of the rehash and of the lookup, against a plain
// restatement of blockchain/service.go:261-269 + :324 that walks block by block over a std::set that
// only grows.  Every array has exactly its size.  Prints counts; exit status 0 iff all agree.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../blockparents_dev.h"

using namespace pz;

namespace {

using Key = std::array<uint8_t, 32>;
constexpr uint64_t kTile = 1024;
std::mt19937_64 rng(20261020);

uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }
Key rnd_key() {
  Key k;
  for (auto& b : k) b = (uint8_t)rng();
  return k;
}

struct Counts {
  uint64_t runs = 0, blocks = 0, saved = 0, refused = 0, closed = 0, linked = 0, in_set = 0, free_ = 0, copies = 0, inserted = 0,
           rehashes = 0, capacity = 0, wraps = 0, lookups = 0;
  uint32_t max_rounds = 0;
} cnt;

[[noreturn]] void die(const char* what, const char* name, uint64_t j) {
  std::printf("MISMATCH %s in '%s' at %llu\n", what, name, (unsigned long long)j);
  std::exit(1);
}

// ---- a received block, as the columns describe it ---------------------------------------------------
struct Blk {
  Key hash;
  std::vector<uint8_t> parent;  // field 1 as received: any length
  uint64_t slot = 10;
  int rows = 1;
  bool last_ok = true, rec_bad = false;
  int32_t status = PZ_OK;  // the decoder's status with CanProcessBlock folded in
};

struct Run {
  uint64_t n = 0, natt = 0, nbytes = 0;
  std::vector<uint8_t> bytes, hash;
  std::vector<uint64_t> bytes_beg, slot, att_first;
  std::vector<uint32_t> bytes_len;
  std::vector<int32_t> block_status, rec_status, att_status;
  bool with_rec = true;
};

Run assemble(const std::vector<Blk>& bl) {
  Run r;
  r.n = bl.size();
  r.bytes_beg.assign(5 * r.n, ~0ull);  // entries 5j+1 .. 5j+4 are not the parent check's: following one trips ASan
  r.bytes_len.assign(5 * r.n, 0xFFFFFFFFu);
  r.att_first.assign(r.n + 1, 0);
  r.with_rec = rnd(4) != 0;
  for (uint64_t j = 0; j < r.n; ++j) {
    const Blk& b = bl[j];
    r.hash.insert(r.hash.end(), b.hash.begin(), b.hash.end());
    r.slot.push_back(b.slot);
    r.block_status.push_back(b.status);
    for (uint64_t g = rnd(3); g; --g) r.bytes.push_back((uint8_t)rng());  // other fields' bytes between
    r.bytes_beg[5 * j] = b.parent.empty() ? rnd(1000) : r.bytes.size();   // (an absent field's beg means nothing)
    r.bytes_len[5 * j] = (uint32_t)b.parent.size();
    r.bytes.insert(r.bytes.end(), b.parent.begin(), b.parent.end());
    for (int k = 0; k < b.rows; ++k) {
      const bool last = k == b.rows - 1;
      static const int32_t other[] = {PZ_ATT_NOT_PROCESSED, 4, 6};
      r.att_status.push_back(last ? (b.last_ok ? PZ_ATT_PROCESSED : other[rnd(3)]) : (rnd(3) ? PZ_ATT_PROCESSED : other[rnd(3)]));
      r.rec_status.push_back(b.rec_bad && k == 0 ? PZ_EINVAL : PZ_OK);
    }
    r.att_first[j + 1] = r.att_status.size();
    if (b.rec_bad) r.with_rec = true;
  }
  r.natt = r.att_status.size();
  r.nbytes = r.bytes.size();
  return r;
}

// ---- the reference, block by block --------------------------------------------------------------------
Key ref_bytes_to_hash(const std::vector<uint8_t>& p) {  // common.BytesToHash
  Key k{};
  const size_t len = p.size() > 32 ? 32 : p.size();
  std::memcpy(k.data() + 32 - len, p.data() + (p.size() - len), len);
  return k;
}

bool ref_open(const Blk& b) { return b.status == PZ_OK && !b.rec_bad && b.rows > 0 && b.last_ok; }  // service.go:272-306

struct Ref {
  std::vector<uint8_t> parent_ok, saved;
  std::set<Key> db;
};

Ref reference(const std::vector<Blk>& bl, const std::vector<Key>& initial) {
  Ref o;
  o.db.insert(initial.begin(), initial.end());
  o.parent_ok.assign(bl.size(), 0), o.saved.assign(bl.size(), 0);
  for (size_t j = 0; j < bl.size(); ++j) {
    const bool ok = bl[j].slot <= 1 || o.db.count(ref_bytes_to_hash(bl[j].parent)) != 0;  // service.go:261-269
    o.parent_ok[j] = ok;
    if (!ok || !ref_open(bl[j])) continue;
    o.saved[j] = 1;
    o.db.insert(bl[j].hash);  // service.go:324
  }
  return o;
}

// ---- the set, sequentially ----------------------------------------------------------------------------
struct Set {
  std::vector<uint32_t> state;
  std::vector<uint8_t> keys;
  uint64_t words[kBsWords] = {0, 0};
  uint32_t cells = 0;
  explicit Set(uint32_t c) : state(c, kBsEmpty), keys(32ull * c, 0), cells(c) {}
};

// pz_bs_insert_kernel: per tile the claims (lanes in a shuffled order), then the leaders' keys, then full.
void seq_insert(Set& t, const uint8_t* hashes, const uint8_t* take, const uint8_t* walk, const uint32_t* flags, uint64_t n,
                uint64_t* count_out) {
  uint32_t s_new = 0, s_over = 0;
  const uint32_t gate_flags = walk && flags ? *flags : 0;
  for (uint64_t t0 = 0; t0 < n; t0 += kTile) {
    const uint64_t m = std::min(kTile, n - t0);
    std::vector<uint32_t> cell(m, 0xFFFFFFFFu), order(m);
    for (uint64_t k = 0; k < m; ++k) order[k] = (uint32_t)k;
    std::shuffle(order.begin(), order.end(), rng);
    for (uint32_t k : order) {
      const uint64_t j = t0 + k;
      if (!(walk ? bp_insert_walked(walk[j], gate_flags) : (!take || take[j] != 0))) continue;
      const Hash32 h = vc_load_hash16(hashes + 32 * j);
      const uint32_t mine = vc_claim((uint32_t)j);
      bool done = false;
      uint32_t c = vc_home(h, t.cells);
      for (uint32_t step = 0; step < t.cells && !done; ++step, c = vc_next(c, t.cells)) {
        if (step && c == 0) ++cnt.wraps;
        const uint32_t v = t.state[c];
        if (v == kBsEmpty) {
          t.state[c] = mine, cell[k] = c;
          break;
        }
        if (v == kBsFull) {
          done = vc_hash_eq(h, vc_load_hash16(t.keys.data() + 32ull * c));
        } else if (bs_is_claim(v)) {
          const uint32_t src = vc_claim_source(v);
          if (src == (uint32_t)j || (src < n && vc_hash_eq(h, vc_load_hash16(hashes + 32ull * src)))) {
            if (mine < v) t.state[c] = mine;
            cell[k] = c, done = true;
          }
        } else {
          die("a cell state that is neither empty, full nor a claim", "insert", c);
        }
      }
      if (!done && cell[k] == 0xFFFFFFFFu) s_over = 1;
    }
    std::vector<uint8_t> lead(m, 0);
    for (uint64_t k = 0; k < m; ++k)
      if (cell[k] != 0xFFFFFFFFu && t.state[cell[k]] == vc_claim((uint32_t)(t0 + k))) {
        lead[k] = 1, ++s_new;
        std::memcpy(t.keys.data() + 32ull * cell[k], hashes + 32 * (t0 + k), 32);
      }
    for (uint64_t k = 0; k < m; ++k)
      if (lead[k]) t.state[cell[k]] = kBsFull;
  }
  t.words[kBsCount] += s_new;
  if (s_over) t.words[kBsErr] |= kBsErrCapacity, ++cnt.capacity;
  if (count_out) *count_out = t.words[kBsCount];
  cnt.inserted += s_new;
}

// pz_bs_rehash_kernel behind reserve().
void seq_reserve(Set& t, uint64_t min_keys) {
  if (2 * min_keys <= t.cells) return;
  Set to(bs_cells(min_keys));
  for (uint32_t c0 = 0; c0 < t.cells; ++c0) {
    if (t.state[c0] != kBsFull) continue;
    const Hash32 h = vc_load_hash16(t.keys.data() + 32ull * c0);
    uint32_t c = vc_home(h, to.cells), step = 0;
    for (; step < to.cells && to.state[c] != kBsEmpty; ++step) c = vc_next(c, to.cells);
    if (step == to.cells) die("no cell in the larger table", "reserve", c0);
    to.state[c] = kBsFull;
    std::memcpy(to.keys.data() + 32ull * c, t.keys.data() + 32ull * c0, 32);
  }
  to.words[kBsCount] = t.words[kBsCount], to.words[kBsErr] = t.words[kBsErr];
  t = to;
  ++cnt.rehashes;
}

std::set<Key> keys_of(const Set& t) {
  std::set<Key> s;
  uint64_t full = 0;
  for (uint32_t c = 0; c < t.cells; ++c) {
    if (t.state[c] == kBsEmpty) continue;
    if (t.state[c] != kBsFull) die("a claim left between calls", "set", c);
    Key k;
    std::memcpy(k.data(), t.keys.data() + 32ull * c, 32);
    if (!s.insert(k).second) die("one key in two cells", "set", c);
    ++full;
  }
  if (full != t.words[kBsCount]) die("the count is not the number of keys", "set", full);
  return s;
}

bool contains(const Set& t, const Key& k) {
  ++cnt.lookups;
  const std::vector<uint8_t> q(k.begin(), k.end());  // exactly 32 bytes
  return bs_contains(t.state.data(), t.keys.data(), t.cells, vc_load_hash16(q.data()));
}

void insert_keys(Set& t, const std::vector<Key>& ks) {
  std::vector<uint8_t> flat;
  for (const Key& k : ks) flat.insert(flat.end(), k.begin(), k.end());
  seq_insert(t, flat.data(), nullptr, nullptr, nullptr, ks.size(), nullptr);
}

// ---- pz_dev_block_parents, sequentially ---------------------------------------------------------------
struct Out {
  std::vector<uint8_t> parent_ok, saved0;
  std::vector<int32_t> status_out;
};

Out seq_parents(const Set& t, const Run& r) {
  const uint64_t n = r.n;
  const int32_t* rec = r.with_rec ? r.rec_status.data() : nullptr;
  // launch 1: open0 and the run table (lanes in a shuffled order: any block may claim a cell first)
  const uint32_t rc = bp_run_cells(n);
  std::vector<uint32_t> run(rc, kBpNoLink), order(n);
  std::vector<uint8_t> open0(n);
  for (uint64_t j = 0; j < n; ++j) order[j] = (uint32_t)j;
  std::shuffle(order.begin(), order.end(), rng);
  for (uint32_t j : order) {
    open0[j] = bp_open0(r.att_first.data(), r.block_status.data(), rec, r.att_status.data(), r.natt, j);
    if (!open0[j]) continue;
    uint32_t c = vc_home(vc_load_hash16(r.hash.data() + 32ull * j), rc), step = 0;
    for (; step < rc && run[c] != kBpNoLink; ++step) c = vc_next(c, rc);
    if (step == rc) die("no cell in the run table", "open", j);
    run[c] = j;
  }
  // launch 2: the words
  std::vector<uint32_t> p(n), a(n), o(n);
  for (uint64_t j = 0; j < n; ++j) {
    const uint64_t beg = r.bytes_beg[5 * j];
    const uint32_t len = r.bytes_len[5 * j];
    uint32_t pw = kBpFalse, sw = kBpFalse;
    if (bp_span_ok(beg, len, r.nbytes)) {
      const bool free = bp_free(r.slot[j]);
      bool in_set = false;
      uint32_t link = kBpNoLink;
      if (!free) {
        const Hash32 parent = bp_parent(r.bytes.data(), beg, len);
        in_set = bs_contains(t.state.data(), t.keys.data(), t.cells, parent);
        if (!in_set) link = bp_link(run.data(), rc, r.hash.data(), parent, j);
      }
      cnt.free_ += free, cnt.in_set += in_set, cnt.linked += link != kBpNoLink;
      pw = bp_parent_word(free, in_set, link);
      sw = bp_saved_word(open0[j] != 0, pw);
    }
    p[j] = pw, a[j] = sw;
  }
  // launch 3: the rounds, double-buffered, then the outputs
  const uint32_t rounds = bp_rounds(n);
  cnt.max_rounds = std::max(cnt.max_rounds, rounds);
  for (uint32_t k = 0; k < rounds; ++k) {
    for (uint64_t j = 0; j < n; ++j) {
      const uint32_t v = a[j];
      if (!bp_resolved(v) && v >= j) die("a link that does not point back", "resolve", j);
      o[j] = bp_jump(v, !bp_resolved(v) && v < n ? a[v] : kBpFalse);
    }
    a.swap(o);
  }
  Out out;
  out.parent_ok.assign(n, 0), out.saved0.assign(n, 0), out.status_out.assign(n, 0);
  for (uint64_t j = 0; j < n; ++j) {
    if (!bp_resolved(a[j])) die("a word the rounds left unresolved", "resolve", j);
    const bool ok = bp_parent_ok(p[j], !bp_resolved(p[j]) && p[j] < n ? a[p[j]] : kBpFalse);
    out.parent_ok[j] = ok, out.saved0[j] = ok && open0[j];
    if (out.saved0[j] != (a[j] == kBpTrue)) die("saved0 against the resolved word", "resolve", j);
    out.status_out[j] = bp_status_out(r.block_status[j], ok);
  }
  return out;
}

// The gate's pass 1 (blockgate.hip) over block_status_out.
uint8_t gate_report(const Run& r, const std::vector<int32_t>& status, uint64_t j) {
  const uint64_t f0 = r.att_first[j], f1 = r.att_first[j + 1];
  if (!bg_span_ok(f0, f1, r.natt)) return kBgRejected;
  uint64_t nproc = 0;
  bool bad = false;
  for (uint64_t i = f0; i < f1; ++i) {
    bad = bad || (r.with_rec && r.rec_status[i] != PZ_OK);
    nproc += r.att_status[i] == PZ_ATT_PROCESSED;
  }
  return bg_report(status[j] == PZ_OK && !bad, f1 - f0, nproc, f1 > f0 ? r.att_status[f1 - 1] : -1);
}

// One run against the reference: the parent check, then the insert after a walk that stops somewhere.
void check(const std::vector<Blk>& bl, const std::vector<Key>& initial, const char* name, uint32_t cells = 0) {
  const Run r = assemble(bl);
  Set t(cells ? cells : bs_cells(initial.size()));
  insert_keys(t, initial);
  const Ref want = reference(bl, initial);
  const Out got = seq_parents(t, r);
  ++cnt.runs, cnt.blocks += r.n;
  for (uint64_t j = 0; j < r.n; ++j) {
    if (got.parent_ok[j] != want.parent_ok[j]) die("parent_ok", name, j);
    if (got.saved0[j] != want.saved[j]) die("saved0", name, j);
    if (got.status_out[j] != (want.parent_ok[j] ? r.block_status[j] : PZ_ENOTFOUND)) die("block_status_out", name, j);
    if ((gate_report(r, got.status_out, j) != kBgRejected) != (got.saved0[j] != 0)) die("the gate's report", name, j);
    cnt.saved += want.saved[j], cnt.refused += !want.parent_ok[j], cnt.closed += want.parent_ok[j] && !want.saved[j];
  }
  // the walk's codes: saved or candidate where the gate opens, deferred from a stop on; rarely a panic
  const uint64_t stop = rnd(3) ? r.n : rnd(r.n + 1);
  const uint32_t flags = rnd(8) == 0 ? kBgPanic : 0;
  std::vector<uint8_t> walk(r.n);
  std::set<Key> db(initial.begin(), initial.end());
  for (uint64_t j = 0; j < r.n; ++j) {
    walk[j] = j >= stop ? kBwDeferred : got.saved0[j] ? (rnd(2) ? kBwSaved : kBwCandidate) : kBwOff;
    if (j < stop && want.saved[j] && !flags) db.insert(bl[j].hash);
  }
  seq_reserve(t, t.words[kBsCount] + r.n);
  uint64_t count = ~0ull;
  seq_insert(t, r.hash.data(), nullptr, walk.data(), &flags, r.n, &count);
  if (t.words[kBsErr]) die("the error word after a reserve", name, 0);
  if (keys_of(t) != db || count != db.size()) die("the set after the insert", name, count);
  for (uint64_t j = 0; j < r.n; ++j) {
    if (contains(t, bl[j].hash) != (db.count(bl[j].hash) != 0)) die("contains(hash)", name, j);
    const Key pk = ref_bytes_to_hash(bl[j].parent);
    if (contains(t, pk) != (db.count(pk) != 0)) die("contains(parent)", name, j);
  }
}

// ---- the cases ------------------------------------------------------------------------------------------
std::vector<uint8_t> vec(const Key& k) { return std::vector<uint8_t>(k.begin(), k.end()); }

// A linear chain: block j's parent is block j - 1, block 0's is `root`.
std::vector<Blk> chain(uint64_t n, const Key& root) {
  std::vector<Blk> bl(n);
  for (uint64_t j = 0; j < n; ++j) {
    bl[j].hash = rnd_key();
    bl[j].parent = vec(j ? bl[j - 1].hash : root);
    bl[j].slot = 2 + j;
    bl[j].rows = 1 + (int)rnd(3);
  }
  return bl;
}

void sized_cases(uint64_t n) {
  const Key root = rnd_key();
  const std::vector<Key> db = {root, rnd_key(), rnd_key()};
  check(chain(n, root), db, "linear chain");                 // the deepest chain: every round is needed
  check(chain(n, rnd_key()), db, "linear chain, unknown root");  // nothing is saved
  if (n >= 2) {
    auto bl = chain(n + 1, root);
    bl.erase(bl.begin() + n / 2);
    check(bl, db, "one block removed");
    bl = chain(n, root);
    std::swap(bl[n / 2], bl[n / 2 - (n / 2 ? 1 : -1)]);
    check(bl, db, "a child before its parent");
    bl = chain(n, root);
    bl[n / 2].last_ok = false;
    check(bl, db, "a closed parent (last attestation refused)");
    bl = chain(n, root);
    bl[n / 3].rows = 0;
    check(bl, db, "a closed parent (no attestation)");
    bl = chain(n, root);
    bl[n / 2].rec_bad = true;
    check(bl, db, "a closed parent (a record not canonical)");
    bl = chain(n, root);
    bl[n - 1 - n / 4].status = 1;
    check(bl, db, "a parent CanProcessBlock refused");
    // delivered twice, the child between and after the copies
    bl = chain(n, root);
    const uint64_t k = n / 2 ? n / 2 - 1 : 0;
    std::vector<Blk> d(bl.begin(), bl.begin() + k + 1);
    if (k + 1 < n) d.push_back(bl[k + 1]);
    d.push_back(bl[k]);
    d.insert(d.end(), bl.begin() + k + 1, bl.end());
    cnt.copies += 2;
    check(d, db, "a block delivered twice");
    // copies whose caller masks differ, in both orders
    for (int first_masked = 0; first_masked < 2; ++first_masked) {
      std::vector<Blk> m(bl.begin(), bl.begin() + k + 1);
      m.back().status = first_masked ? 1 : PZ_OK;
      if (k + 1 < n) m.push_back(bl[k + 1]);
      m.push_back(bl[k]);
      m.back().status = first_masked ? PZ_OK : 1;
      m.insert(m.end(), bl.begin() + k + 1, bl.end());
      cnt.copies += 2;
      check(m, db, first_masked ? "copies: masked then open" : "copies: open then masked");
    }
    // a copy whose own parent arrives only between the copies: the later copy saves, the earlier did not
    if (k >= 1) {
      std::vector<Blk> m(bl.begin(), bl.begin() + k - 1);
      m.push_back(bl[k]), m.push_back(bl[k - 1]), m.push_back(bl[k]);
      m.insert(m.end(), bl.begin() + k + 1, bl.end());
      cnt.copies += 2;
      check(m, db, "a copy before and after its own parent");
    }
  }
  if (n >= 1) {
    auto bl = chain(n, rnd_key());  // slots 0 and 1 need no parent; their children link to them
    for (uint64_t j = 0; j < n; j += 5) bl[j].slot = (j / 5) % 2;
    check(bl, db, "slots 0 and 1");
    // parent spans of length 0, 31, 32 and 33; block 2 carries the zero hash, which block 3's absent
    // field names (one block only: equal hashes are equal blocks)
    bl = chain(n, root);
    Key zero{};
    for (uint64_t j = 1; j < n; ++j) {
      if (j % 4 == 1) bl[j - 1].hash[0] = 0;  // a leading zero byte: the 31-byte form exists
      if (j == 3) bl[j - 1].hash = zero;
    }
    for (uint64_t j = 1; j < n; ++j) {
      const Key target = bl[j - 1].hash;
      bl[j].parent = vec(target);
      if (j % 4 == 1) bl[j].parent.erase(bl[j].parent.begin());                         // 31 bytes, right-aligned
      if (j % 4 == 2) bl[j].parent.insert(bl[j].parent.begin(), (uint8_t)(1 + rnd(255)));  // 33 bytes: the last 32 count
      if (j == 3) bl[j].parent.clear();                                                 // absent: the zero hash
    }
    check(bl, db, "parent spans of 0, 31, 32 and 33 bytes");
    auto z = chain(n, zero);
    z[0].parent.clear();
    check(z, {zero, root}, "the zero hash in the set");
    check(z, {root}, "the zero hash not in the set");
  }
}

Key homed(uint8_t home, uint64_t tag) {  // a key whose home cell in a table of <= 256 cells is `home`
  Key k = rnd_key();
  k[0] = home;
  std::memcpy(k.data() + 8, &tag, 8);
  return k;
}

void table_cases() {
  {  // 8 cells, keys sharing home 6: the probes wrap past cell 7
    Set t(8);
    std::vector<Key> ks = {homed(6, 1), homed(6, 2), homed(6, 3), homed(6, 4), Key{}};
    insert_keys(t, ks);
    insert_keys(t, ks);  // again: nothing changes
    ks.push_back(homed(6, 5));
    insert_keys(t, {ks[1], ks[1], ks[5], ks[1], ks[5]});  // duplicates inside one call count once
    if (keys_of(t) != std::set<Key>(ks.begin(), ks.end()) || t.words[kBsCount] != 6) die("same-home keys", "8 cells", 0);
    for (const Key& k : ks)
      if (!contains(t, k)) die("contains", "8 cells", 0);
    if (contains(t, homed(6, 9)) || contains(t, homed(3, 1))) die("contains(absent)", "8 cells", 0);
    // full: two more fit, the ninth does not, and a lookup of an absent key in a full table ends
    insert_keys(t, {homed(1, 6), homed(2, 7)});
    if (t.words[kBsCount] != 8 || t.words[kBsErr]) die("eight keys in eight cells", "8 cells", 0);
    if (contains(t, homed(5, 10))) die("contains(absent) in a full table", "8 cells", 0);
    const Key ninth = homed(4, 8);
    insert_keys(t, {ninth});
    if (t.words[kBsCount] != 8 || !(t.words[kBsErr] & kBsErrCapacity) || contains(t, ninth)) die("the capacity bit", "8 cells", 0);
    t.words[kBsErr] = 0;
    const std::set<Key> before = keys_of(t);
    seq_reserve(t, 2048);  // 8 -> 4,096 cells
    if (t.cells != 4096 || keys_of(t) != before) die("reserve 8 -> 4096", "8 cells", t.cells);
    seq_reserve(t, 100);  // no-op
    if (t.cells != 4096) die("reserve shrank", "8 cells", t.cells);
    insert_keys(t, {ninth});
    if (t.words[kBsCount] != 9 || t.words[kBsErr] || !contains(t, ninth)) die("the ninth key after the reserve", "8 cells", 0);
  }
  {  // take: only the chosen become keys
    Set t(64);
    std::vector<uint8_t> flat, take;
    std::set<Key> want;
    for (int k = 0; k < 20; ++k) {
      const Key key = rnd_key();
      flat.insert(flat.end(), key.begin(), key.end());
      take.push_back(k % 3 == 0);
      if (k % 3 == 0) want.insert(key);
    }
    seq_insert(t, flat.data(), take.data(), nullptr, nullptr, 20, nullptr);
    if (keys_of(t) != want) die("take", "insert", 0);
  }
  if (bs_cells(0) != 8 || bs_cells(4) != 8 || bs_cells(5) != 16 || bs_cells(1u << 30) != (1u << 31)) die("bs_cells", "table", 0);
  if (bp_run_cells(0) != 2 || bp_run_cells(3) != 8 || bp_run_cells((1ull << 31) - 1) != (1u << 31)) die("bp_run_cells", "table", 0);
  if (bp_rounds(0) != 0 || bp_rounds(1) != 0 || bp_rounds(2) != 1 || bp_rounds(1024) != 10 || bp_rounds(1025) != 11) die("bp_rounds", "table", 0);
}

// Random runs over a small universe of blocks, so that copies, forks, early children and closed
// parents mix; some in an 8-cell set whose keys share a home cell.
void random_runs(int count) {
  for (int it = 0; it < count; ++it) {
    const uint64_t universe = 2 + rnd(24), n = rnd(40);
    const bool tiny = rnd(4) == 0;
    std::vector<Blk> u(universe);
    std::vector<Key> db;
    for (uint64_t k = 0; k < (tiny ? 3 : 1 + rnd(6)); ++k) db.push_back(tiny ? homed(7, k) : rnd_key());
    for (uint64_t k = 0; k < universe; ++k) {
      u[k].hash = tiny ? homed(7, 100 + k) : rnd_key();
      const uint64_t pick = rnd(10);
      const Key par = pick < 6 && k ? u[rnd(k)].hash : pick < 8 ? db[rnd(db.size())] : rnd_key();
      u[k].parent = vec(par);
      if (rnd(8) == 0) u[k].parent.insert(u[k].parent.begin(), (uint8_t)rng());
      u[k].slot = rnd(12) == 0 ? rnd(2) : 2 + rnd(100);
      u[k].rows = (int)rnd(4);
      u[k].last_ok = rnd(6) != 0;
      u[k].rec_bad = rnd(12) == 0;
    }
    std::vector<Blk> bl;
    for (uint64_t j = 0; j < n; ++j) {
      bl.push_back(u[rnd(4) ? std::min(universe - 1, j * universe / (n ? n : 1) + rnd(3)) : rnd(universe)]);
      bl.back().status = rnd(7) == 0 ? 1 : PZ_OK;  // CanProcessBlock differs from delivery to delivery
    }
    check(bl, db, "random", tiny ? 8 : 0);
  }
}

}  // namespace

int main() {
  for (uint64_t n : {0ull, 1ull, 2ull, 63ull, 64ull, 65ull, 1023ull, 1024ull, 1025ull, 2049ull}) sized_cases(n);
  table_cases();
  random_runs(4000);
  std::printf("ok: %llu runs, %llu blocks, %llu saved, %llu refused, %llu closed, %llu linked, %llu in-set, %llu free, %llu copies, "
              "%llu inserted, %llu rehashes, %llu capacity, %llu wraps, %llu lookups, %u rounds\n",
              (unsigned long long)cnt.runs, (unsigned long long)cnt.blocks, (unsigned long long)cnt.saved,
              (unsigned long long)cnt.refused, (unsigned long long)cnt.closed, (unsigned long long)cnt.linked,
              (unsigned long long)cnt.in_set, (unsigned long long)cnt.free_, (unsigned long long)cnt.copies,
              (unsigned long long)cnt.inserted, (unsigned long long)cnt.rehashes, (unsigned long long)cnt.capacity,
              (unsigned long long)cnt.wraps, (unsigned long long)cnt.lookups, cnt.max_rounds);
  return 0;
}
