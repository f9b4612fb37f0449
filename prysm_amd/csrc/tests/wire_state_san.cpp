// The two states' encoding rules (wire_state_dev.h) on the CPU under ASan+UBSan: the inlines the
// kernels of wire_state.hip compile, driven through a sequential form of their phases (plan, size,
// scan, write; head right-aligned at its bound, tail behind the validators; the recent hashes) into
// buffers of exactly the encoded size, against a byte-by-byte scalar encoder that builds every
// message bottom-up.  Cases: tests/state_wire_cases.py's list written out below, then random tables,
// heads and hash lists.  Built by `make -C prysm_amd/csrc san_wirestate`; no GPU code involved.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../wire_state_dev.h"

using namespace pz;
typedef std::vector<uint8_t> Bytes;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

// ---- the scalar encoder ---------------------------------------------------------------------------
static void r_varint(Bytes& o, uint64_t x) {
  for (;;) {
    const uint8_t b = x & 0x7f;
    x >>= 7;
    if (x) o.push_back(b | 0x80);
    else {
      o.push_back(b);
      return;
    }
  }
}
static void r_u(Bytes& o, uint32_t field, uint64_t v) {
  if (!v) return;
  r_varint(o, (uint64_t)field << 3);
  r_varint(o, v);
}
static void r_msg(Bytes& o, uint32_t field, const Bytes& body) {
  r_varint(o, ((uint64_t)field << 3) | 2);
  r_varint(o, body.size());
  o.insert(o.end(), body.begin(), body.end());
}
static void r_bytes(Bytes& o, uint32_t field, const Bytes& b) {
  if (!b.empty()) r_msg(o, field, b);
}

struct Table {
  std::vector<uint64_t> arr_offs{0};
  std::vector<uint64_t> arr_shard;
  std::vector<uint32_t> arr_comm;
  std::vector<std::vector<uint32_t>> comms;
  void array(const std::vector<std::pair<uint64_t, uint32_t>>& entries) {
    for (auto& e : entries) arr_shard.push_back(e.first), arr_comm.push_back(e.second);
    arr_offs.push_back(arr_shard.size());
  }
};

static Bytes r_table(const Table& t, uint32_t field) {
  Bytes out;
  for (size_t a = 0; a + 1 < t.arr_offs.size(); ++a) {
    Bytes body;
    for (uint64_t e = t.arr_offs[a]; e < t.arr_offs[a + 1]; ++e) {
      Bytes sc, packed;
      r_u(sc, 1, t.arr_shard[e]);
      for (uint32_t m : t.comms[t.arr_comm[e]]) r_varint(packed, m);
      r_bytes(sc, 2, packed);
      r_msg(body, 1, sc);
    }
    if (field) r_msg(out, field, body);
    else out.insert(out.end(), body.begin(), body.end());
  }
  return out;
}

// ---- the kernels' phases, one after the other ---------------------------------------------------------
static uint64_t g_tables = 0, g_heads = 0, g_recents = 0;

static void run_table(const Table& t, uint32_t field) {
  const size_t narr = t.arr_offs.size() - 1, nent = t.arr_shard.size();
  // plan: the chunks' prefix
  std::vector<uint64_t> chunk_first(nent + 1, 0);
  for (size_t e = 0; e < nent; ++e) chunk_first[e + 1] = chunk_first[e] + ws_chunks(t.comms[t.arr_comm[e]].size());
  const uint64_t nch = chunk_first[nent];
  // size: every chunk's bytes; scan: their prefix
  std::vector<uint64_t> chunk_pre(nch + 1, 0);
  for (size_t e = 0; e < nent; ++e) {
    const auto& c = t.comms[t.arr_comm[e]];
    for (uint64_t k = chunk_first[e]; k < chunk_first[e + 1]; ++k) {
      const size_t lo = (k - chunk_first[e]) * kWsChunk, hi = std::min<size_t>(c.size(), lo + kWsChunk);
      uint64_t s = 0;
      for (size_t i = lo; i < hi; ++i) s += ws_vlen(c[i]);
      chunk_pre[k + 1] = chunk_pre[k] + s;
    }
  }
  std::vector<uint64_t> entry_pre(nent + 1, 0), packed(nent, 0);
  for (size_t e = 0; e < nent; ++e) {
    packed[e] = chunk_pre[chunk_first[e + 1]] - chunk_pre[chunk_first[e]];
    entry_pre[e + 1] = entry_pre[e] + ws_entry_framed(t.arr_shard[e], packed[e]);
  }
  std::vector<uint64_t> arr_adj(narr, 0), arr_body(narr, 0);
  uint64_t total = 0;
  for (size_t a = 0; a < narr; ++a) {
    const uint64_t first = entry_pre[t.arr_offs[a]];
    arr_body[a] = entry_pre[t.arr_offs[a + 1]] - first;
    const uint64_t head = ws_array_head_len(field, arr_body[a]);
    arr_adj[a] = total + head - first;
    total += head + arr_body[a];
  }
  const Bytes want = r_table(t, field);
  CHECK(total == want.size());
  // write, into exactly `total` bytes
  std::unique_ptr<uint8_t[]> out(new uint8_t[total ? total : 1]);
  std::memset(out.get(), 0xA5, total);
  for (size_t a = 0; a < narr; ++a) {
    const uint64_t first = entry_pre[t.arr_offs[a]];
    const uint32_t head = ws_array_head_len(field, arr_body[a]);
    CHECK(ws_put_array_head(out.get() + arr_adj[a] + first - head, field, arr_body[a]) == head);
    for (uint64_t e = t.arr_offs[a]; e < t.arr_offs[a + 1]; ++e) {
      uint8_t* p = out.get() + entry_pre[e] + arr_adj[a];
      const uint32_t eh = ws_entry_head_len(t.arr_shard[e], packed[e]);
      CHECK(ws_put_entry_head(p, t.arr_shard[e], packed[e]) == eh);
      const auto& c = t.comms[t.arr_comm[e]];
      for (uint64_t k = chunk_first[e]; k < chunk_first[e + 1]; ++k) {
        uint8_t* q = p + eh + (chunk_pre[k] - chunk_pre[chunk_first[e]]);
        const size_t lo = (k - chunk_first[e]) * kWsChunk, hi = std::min<size_t>(c.size(), lo + kWsChunk);
        for (size_t i = lo; i < hi; ++i) q += ws_put(q, c[i]);
      }
    }
  }
  CHECK(total == 0 || std::memcmp(out.get(), want.data(), total) == 0);
  ++g_tables;
}

struct Rec {
  uint64_t dynasty, slot;
  Bytes hash;
};
struct Head {
  uint64_t v[8];  // fields 1-5, 7 (the handle's), 6, 9
  Bytes seed;
  std::vector<Rec> recs;
  uint32_t stride;
};

static void run_head(const Head& h, const Bytes& validators, const Bytes& tail) {
  Bytes want;
  const uint32_t fields[8] = {1, 2, 3, 4, 5, 7, 6, 9};
  uint64_t by_field[10] = {};
  for (int k = 0; k < 8; ++k) by_field[fields[k]] = h.v[k];
  for (uint32_t f = 1; f <= 7; ++f) r_u(want, f, by_field[f]);
  r_bytes(want, 8, h.seed);
  r_u(want, 9, by_field[9]);
  for (const Rec& r : h.recs) {
    Bytes body;
    r_u(body, 1, r.dynasty);
    r_bytes(body, 2, r.hash);
    r_u(body, 3, r.slot);
    r_msg(want, 10, body);
  }
  const size_t head_want = want.size();
  want.insert(want.end(), validators.begin(), validators.end());
  want.insert(want.end(), tail.begin(), tail.end());

  WsHeadScalars s;
  for (int f = 0; f < 10; ++f) s.f[f] = by_field[f];
  s.seed_len = (uint32_t)h.seed.size();
  const uint64_t H = ws_head_bound((uint32_t)h.recs.size(), h.stride);
  uint64_t head_len = ws_head_scalars_size(s);
  for (const Rec& r : h.recs) head_len += ws_record_framed(r.dynasty, (uint32_t)r.hash.size(), r.slot);
  CHECK(head_len == head_want && head_len <= H && H % 16 == 0);
  const uint64_t begin = ws_span_begin(H, head_len), total = H + validators.size() + tail.size();
  std::unique_ptr<uint8_t[]> out(new uint8_t[total ? total : 1]);  // exactly the head bound and what follows it
  std::memset(out.get(), 0xA5, total);
  uint8_t* p = out.get() + begin;
  p += ws_put_head_scalars(p, s, h.seed.data());
  for (const Rec& r : h.recs) {
    const uint32_t n = ws_put_record(p, r.dynasty, r.hash.data(), (uint32_t)r.hash.size(), r.slot);
    CHECK(n == ws_record_framed(r.dynasty, (uint32_t)r.hash.size(), r.slot));
    p += n;
  }
  CHECK(p == out.get() + H);
  if (!validators.empty()) std::memcpy(out.get() + H, validators.data(), validators.size());
  if (!tail.empty()) std::memcpy(out.get() + ws_tail_begin(H, validators.size()), tail.data(), tail.size());
  CHECK(ws_span_len(head_len, validators.size(), tail.size()) == want.size());
  CHECK(want.empty() || std::memcmp(out.get() + begin, want.data(), want.size()) == 0);
  for (uint64_t k = 0; k < begin; ++k) CHECK(out[k] == 0xA5);
  ++g_heads;
}

static void run_recent(const std::vector<Bytes>& rows, const std::vector<uint8_t>* lens) {
  Bytes want;
  uint64_t total = 0;
  for (size_t i = 0; i < rows.size(); ++i) {
    const uint32_t n = lens ? (*lens)[i] : 32;
    r_msg(want, 2, Bytes(rows[i].end() - n, rows[i].end()));
    total += ws_recent_size(n);
  }
  CHECK(total == want.size());
  std::unique_ptr<uint8_t[]> out(new uint8_t[total ? total : 1]);
  uint8_t* p = out.get();
  for (size_t i = 0; i < rows.size(); ++i) p += ws_put_recent(p, rows[i].data(), lens ? (*lens)[i] : 32);
  CHECK(p == out.get() + total && (total == 0 || std::memcmp(out.get(), want.data(), total) == 0));
  ++g_recents;
}

// ---- the cases -------------------------------------------------------------------------------------
static std::vector<uint32_t> small(size_t n, size_t first = 0) {
  std::vector<uint32_t> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = (uint32_t)((i + first) % 128);
  return v;
}

static const size_t kSizes[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4097, 16384, 70001};
static const uint32_t kEdges[] = {0, 127, 128, 16383, 16384, 2097151, 2097152, 268435455, 268435456, 0xFFFFFFFFu};
static const uint64_t kShards[] = {0, 1, 127, 128, ~0ull};

static void listed_tables() {
  const uint32_t fields[] = {12, 0, 1, 16, (1u << 29) - 1};
  for (uint32_t field : fields) {
    Table sizes, one;
    std::vector<std::pair<uint64_t, uint32_t>> all;
    for (size_t n : kSizes) {
      sizes.comms.push_back(small(n, n));
      sizes.array({{5, (uint32_t)sizes.comms.size() - 1}});
      one.comms.push_back(small(n));
      all.push_back({one.comms.size() - 1, (uint32_t)one.comms.size() - 1});
    }
    one.array(all);
    run_table(sizes, field);
    run_table(one, field);
    Table edges;
    for (uint32_t v : kEdges) {
      edges.comms.push_back({v});
      edges.array({{3, (uint32_t)edges.comms.size() - 1}});
    }
    std::vector<uint32_t> many;
    for (int r = 0; r < 30; ++r) many.insert(many.end(), std::begin(kEdges), std::end(kEdges));
    edges.comms.push_back(many);
    edges.array({{4, (uint32_t)edges.comms.size() - 1}, {0, 0}});
    run_table(edges, field);
    Table shards;
    shards.comms = {small(0), small(3)};
    for (uint64_t s : kShards) shards.array({{s, 0}, {s, 1}});
    run_table(shards, field);
    Table lengths;  // ShardAndCommittee bodies of 127 / 128 / 16,383 / 16,384 bytes
    for (size_t n : {125, 126, 16380, 16381}) {
      lengths.comms.push_back(small(n));
      lengths.array({{0, (uint32_t)lengths.comms.size() - 1}});
    }
    run_table(lengths, field);
    Table framed;  // single entries of 127 / 128 / 16,383 / 16,384 bytes framed
    for (size_t n : {123, 124, 16377, 16378}) {
      framed.comms.push_back(small(n));
      framed.array({{0, (uint32_t)framed.comms.size() - 1}});
    }
    run_table(framed, field);
    Table bodies;  // array bodies of the same four lengths
    bodies.comms = {small(123), small(122), small(0), small(16377), small(16378)};
    bodies.array({{0, 0}});
    bodies.array({{0, 1}, {0, 2}});
    bodies.array({{0, 3}});
    bodies.array({{0, 4}});
    run_table(bodies, field);
    Table empties;
    empties.comms = {small(2)};
    empties.array({});
    empties.array({{1, 0}});
    empties.array({});
    empties.array({});
    run_table(empties, field);
    run_table(Table(), field);  // narr 0
    Table none;
    none.array({});
    run_table(none, field);
    Table empty_entry;
    empty_entry.comms = {small(0)};
    empty_entry.array({{0, 0}});
    run_table(empty_entry, field);
    Table shared;
    shared.comms = {small(300), small(1)};
    shared.array({{7, 0}, {8, 0}});
    shared.array({{9, 1}, {7, 0}, {0, 1}});
    run_table(shared, field);
    Table wide;  // narr 128; the genesis shape: every array one entry over a slice of the validators
    for (uint32_t a = 0; a < 128; ++a) {
      wide.comms.push_back(small(16, 8 * a));
      wide.array({{a % 7, a}});
    }
    run_table(wide, field);
  }
}

static void listed_heads() {
  const uint64_t M = ~0ull;
  const Bytes val = {0x5a, 0x00, 0x5a, 0x02, 0x28, 0x20}, tail = {0x62, 0x00};
  for (uint64_t v : {uint64_t(0), uint64_t(1), M}) run_head(Head{{v, v, v, v, v, v, v, v}, {}, {}, 32}, val, tail);
  for (int k = 0; k < 8; ++k) {
    Head h{{}, {}, {}, 32};
    h.v[k] = M;
    run_head(h, {}, {});
  }
  for (size_t n : {0, 32, 64}) run_head(Head{{1, 0, M, 0, 1, M, 0, 1}, Bytes(n, 0x7e), {{3, 9, Bytes(32, 1)}}, 32}, val, {});
  run_head(Head{{}, {}, std::vector<Rec>(5, Rec{0, 0, {}}), 32}, {}, tail);
  Head lens{{128, 2, 64, 0, 1, 1ull << 40, 9, 0}, Bytes(32, 9), {}, 32};
  for (size_t n : {0, 1, 31, 32}) lens.recs.push_back(Rec{n + 1, M, Bytes(n, (uint8_t)n)});
  run_head(lens, val, tail);
  Head wide{{128, 2, 64, 0, 1, 1ull << 40, 0, 7}, {}, {}, 48};
  for (size_t n : {33, 48, 0, 32}) wide.recs.push_back(Rec{M, n, Bytes(n, 0xee)});
  run_head(wide, val, tail);
  Head many{{M, 3, 5, 1, 0, 77, 1023, 0}, Bytes(64, 0x11), {}, 32};
  for (uint64_t s = 0; s < 1024; ++s) many.recs.push_back(Rec{s % 3, (s % 5) << (s % 50), Bytes(s % 33, (uint8_t)s)});
  run_head(many, val, tail);
  Head full{{M, M, M, M, M, M, M, M}, Bytes(64, 0xff), std::vector<Rec>(7, Rec{M, M, Bytes(256, 0xff)}), 256};  // the bound is met
  run_head(full, {}, {});
}

int main() {
  for (uint64_t x : {0ull, 1ull, 127ull, 128ull, 16383ull, 16384ull, (1ull << 63), ~0ull}) {
    Bytes want;
    r_varint(want, x);
    uint8_t buf[10];
    CHECK(ws_vlen(x) == want.size() && ws_put(buf, x) == want.size() && std::memcmp(buf, want.data(), want.size()) == 0);
  }
  listed_tables();
  listed_heads();
  std::mt19937_64 rng(7);
  for (int it = 0; it < 3000; ++it) {  // random tables
    Table t;
    const int ncomm = 1 + rng() % 6;
    for (int c = 0; c < ncomm; ++c) {
      const size_t n = rng() % 4 == 0 ? rng() % 700 : rng() % 9;
      std::vector<uint32_t> m(n);
      for (auto& x : m) x = (uint32_t)(rng() >> (32 + rng() % 32));
      t.comms.push_back(m);
    }
    const int narr = rng() % 6;
    for (int a = 0; a < narr; ++a) {
      std::vector<std::pair<uint64_t, uint32_t>> ents(rng() % 4);
      for (auto& e : ents) e = {rng() % 3 == 0 ? 0 : rng() >> (rng() % 64), (uint32_t)(rng() % ncomm)};
      t.array(ents);
    }
    run_table(t, it % 5 == 0 ? 0 : it % 5 == 1 ? 12 : (uint32_t)(rng() % ((1u << 29) - 1)) + 1);
  }
  for (int it = 0; it < 2000; ++it) {  // random heads and hash lists
    const uint32_t stride = 32 + 16 * (rng() % 15);
    Head h{{}, Bytes(rng() % 65, (uint8_t)rng()), {}, stride};
    for (auto& v : h.v) v = rng() % 3 == 0 ? 0 : rng() >> (rng() % 64);
    h.recs.resize(rng() % 12);
    for (auto& r : h.recs) r = Rec{rng() % 2 ? 0 : rng() >> (rng() % 64), rng() % 2 ? 0 : rng() >> (rng() % 64), Bytes(rng() % (stride + 1), (uint8_t)rng())};
    run_head(h, Bytes(rng() % 40, 0x5a), Bytes(rng() % 40, 0x62));
    std::vector<Bytes> rows(rng() % 20, Bytes(32));
    std::vector<uint8_t> rl(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) {
      for (auto& b : rows[i]) b = (uint8_t)rng();
      rl[i] = (uint8_t)(rng() % 33);
    }
    run_recent(rows, it % 2 ? &rl : nullptr);
  }
  const std::vector<uint8_t> genesis_lens(128, 0);  // types/state.go:46-57: 128 empty hashes
  run_recent(std::vector<Bytes>(128, Bytes(32, 0)), &genesis_lens);
  std::printf("ok: %llu tables, %llu heads, %llu hash lists\n", (unsigned long long)g_tables, (unsigned long long)g_heads,
              (unsigned long long)g_recents);
  return 0;
}
