// Native self-test of the host runtime, built with AddressSanitizer + UBSan by
// ``python -m biscotti_amd._build --sanitize`` and with ThreadSanitizer by ``--tsan`` (host code only: GPU
// sanitizers are not used).  It drives every runtime module from several threads at once and checks known
// answers, and stresses the thread pool and job dispatcher the bindings run their batches on (overlapping
// jobs from several submitting threads, jobs that wait on earlier jobs), so memory errors, UB and data races
// that the Python tests cannot see show up here.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <future>
#include <thread>
#include <vector>

#include "bn256.hpp"
#include "fixed_base.h"
#include "hash.hpp"
#include "keys.hpp"
#include "ledger.hpp"
#include "msm_lanes.h"
#include "pairing.hpp"
#include "pool.hpp"
#include "protocol.hpp"
#include "shares.hpp"
#include "vrf.hpp"

using namespace bsc;

static std::atomic<int> failures{0};
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static void test_hash() {
  const Bytes abc = {'a', 'b', 'c'};
  CHECK(hex(Sha256::digest(abc)) == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
  Bytes big(100000);
  for (size_t i = 0; i < big.size(); ++i) big[i] = u8(i * 7);
  Sha256 inc;
  inc.update(big.data(), 333);
  inc.update(big.data() + 333, big.size() - 333);
  u8 a[32];
  inc.final(a);
  CHECK(Bytes(a, a + 32) == Sha256::digest(big));
  CHECK(hex(Sha512::digest(abc)).rfind("ddaf35a193617aba", 0) == 0);
}

static void test_curve() {
  const G1 g = G1::generator();
  const G1 a = g.mul_i64(123456789), b = g.mul_i64(-987654321);
  CHECK(a.add(b).equals(g.mul_i64(123456789 - 987654321)));
  CHECK(G1::unmarshal(a.marshal()).equals(a));
  CHECK(g.add(g.neg()).is_inf());
  const G2 h = G2::generator();
  CHECK(h.add(h).equals(h.dbl()));
  CHECK(G2::unmarshal(h.dbl().marshal()).equals(h.dbl()));
  const Scalar sk = Scalar::from_i64(424242);
  const G1 pk = g.mul(sk.v);
  const Bytes msg = {1, 2, 3, 4};
  const Bytes sig = schnorr_sign(msg, sk, Bytes(32, 7));
  CHECK(schnorr_verify(msg, pk, sig));
  CHECK(!schnorr_verify(Bytes{1, 2, 3, 5}, pk, sig));
}

static void test_pairing() {
  const G1 g = G1::generator();
  const G2 h = G2::generator();
  const Fp12 e = pairing(g, h);
  CHECK(!e.is_one());
  CHECK(pairing(g.mul_i64(6), h) == e.pow(U256::from_u64(6)));
}

static void test_vrf() {
  const Bytes seed = {0x9d, 0x61, 0xb1, 0x9d, 0xef, 0xfd, 0x5a, 0x60, 0xba, 0x84, 0x4a, 0xf4, 0x92, 0xec, 0x2c, 0xc4,
                      0x44, 0x49, 0xc5, 0x69, 0x7b, 0x32, 0x69, 0x19, 0x70, 0x3b, 0xac, 0x03, 0x1c, 0xae, 0x7f, 0x60};
  const auto out = vrf_prove(VrfKey::cached(seed), Bytes());
  CHECK(hex(out.second).rfind("8657106690b5526245a92b003bb079cc", 0) == 0);
  Bytes beta;
  CHECK(vrf_verify(VrfKey::cached(seed).pk, Bytes(), out.second, &beta) && beta == out.first);
}

static void test_shares_and_ledger() {
  const std::vector<G1> pk = gen_commit_key_g1(23, Scalar::from_i64(2));
  std::vector<i64> c(23);
  for (int i = 0; i < 23; ++i) c[size_t(i)] = (i * 7919) % 2001 - 1000;
  const SharePackage sp = make_shares(c, pk, 10, 21);
  CHECK(sp.commitment.equals(commit(c, pk, 0)));
  const std::vector<i64> xs = share_xs(21);
  for (int k = 0; k < 3; ++k) {
    std::vector<i64> ys(sp.ys.begin() + 21 * k, sp.ys.begin() + 21 * (k + 1)), got;
    CHECK(recover_exact(xs, ys, 9, &got));
    for (int j = 0; j < 10 && 10 * k + j < 23; ++j) CHECK(got[size_t(j)] == c[size_t(10 * k + j)]);
  }
  Blockchain chain = Blockchain::with_genesis(5);
  for (int it = 0; it < 3; ++it) {
    BlockData d;
    d.iteration = it;
    d.global_w = {0.5 * it, -1.25, 3.0, 1e-7, 2.0};
    Update u;
    u.iteration = it;
    u.commitment = sp.commitment.marshal();
    u.accepted = true;
    d.deltas.push_back(u);
    chain.append(chain.make_block(d, {{0, 10}, {1, 15}}, 1000 + it));
  }
  CHECK(chain.verify());
  CHECK(!chain.print_chain().empty());
}

// The chain audit's array view of a chain: every kind of block, a commitment of the wrong length, a delta
// vector of the wrong length, a model of the wrong width, an empty range, and the strict marshal check.
static void test_chain_audit_arrays() {
  const size_t d = 5;
  const std::vector<G1> pk = gen_commit_key_g1(d, Scalar::from_i64(2));
  const Bytes cm = commit({3, -4, 0, 1ll << 33, 7}, pk, 0).marshal();
  Blockchain chain = Blockchain::with_genesis(d);
  auto add = [&](std::vector<double> w, std::vector<Update> us, i64 it) {
    BlockData bd;
    bd.iteration = it;
    bd.global_w = std::move(w);
    bd.deltas = std::move(us);
    chain.append(chain.make_block(bd, {{0, 10}}, 1000 + it));
  };
  Update sec;
  sec.commitment = cm;
  sec.accepted = true;
  Update shortc = sec;
  shortc.commitment.resize(63);
  Update plain = sec;
  plain.delta = {1, 2, 3, 4, 5};
  Update plain_short = sec;
  plain_short.delta = {1, 2};
  plain_short.accepted = false;
  Update bare;
  add({1, 2, 3, 4, 5}, {sec, shortc}, 0);          // SECAGG, second commitment of 63 bytes
  add({1, 2, 3, 4, 5}, {}, 1);                     // EMPTY
  add({2, 4, 6, 8, 10}, {plain, plain_short}, 2);  // PLAIN, second vector of 2 entries
  add({2, 4, 6}, {bare}, 3);                       // NONE, and a model of the wrong width
  const AuditArrays a = chain.audit_arrays(d, 1, 99);
  CHECK(a.first == 1 && a.kind.size() == 4 && a.models.size() == 5 * d);
  CHECK(a.kind[0] == AuditArrays::SECAGG && a.kind[1] == AuditArrays::EMPTY && a.kind[2] == AuditArrays::PLAIN &&
        a.kind[3] == AuditArrays::NONE);
  CHECK((a.offsets == std::vector<int32_t>{0, 2, 2, 4, 4}));
  CHECK(a.commits.size() == 4 * 64 && a.flags.size() == 4);
  CHECK(a.flags[0] == (AuditArrays::ACCEPTED | AuditArrays::LEN_OK) && a.flags[1] == AuditArrays::ACCEPTED);
  CHECK(a.flags[2] == (AuditArrays::ACCEPTED | AuditArrays::LEN_OK | AuditArrays::VEC_OK));
  CHECK(a.flags[3] == AuditArrays::LEN_OK);
  CHECK(std::memcmp(a.commits.data(), cm.data(), 64) == 0);
  for (size_t i = 64; i < 128; ++i) CHECK(a.commits[i] == 0);
  CHECK((a.plain_update == std::vector<int32_t>{2, 3}) && a.plain_delta.size() == 2 * d);
  CHECK(a.plain_delta[4] == 5.0 && a.plain_delta[d] == 0.0);
  CHECK(a.models[0] == 0.0 && a.models[d + 4] == 5.0 && a.models[4 * d] != a.models[4 * d]);   // NaN row
  const AuditArrays part = chain.audit_arrays(d, 3, 4);
  CHECK(part.first == 3 && part.kind.size() == 1 && part.models.size() == 2 * d && part.flags.size() == 2);
  const AuditArrays none = chain.audit_arrays(d, 5, 9);
  CHECK(none.kind.empty() && none.models.empty() && none.offsets.size() == 1);
  CHECK(G1::marshaled_valid(cm.data()));
  CHECK(G1::marshaled_valid(Bytes(64, 0).data()));
  Bytes bad = cm;
  bad[63] ^= 1;
  CHECK(!G1::marshaled_valid(bad.data()));
  Bytes big = cm;   // x + p: the same point to a reducing decoder, refused by the strict one
  U256 xp;
  add_u256(xp, U256::from_be(cm.data()), PRIME());
  xp.to_be(big.data());
  if (cmp(xp, PRIME()) >= 0 && cmp(xp, U256::from_be(cm.data())) > 0) CHECK(!G1::marshaled_valid(big.data()));
}

static void test_protocol() {
  ProtocolConfig pc;
  pc.num_nodes = 30;
  pc.derive();
  std::map<i64, i64> stake;
  for (i64 i = 0; i < 30; ++i) stake[i] = 10 + 5 * (i % 4);
  std::vector<i64> v, m;
  select_roles(stake, Sha256::digest(Bytes{9}), 3, 3, 30, &v, &m);
  CHECK(v.size() == 3 && m.size() == 3);
  CHECK(select_noisers(stake, Sha256::digest(Bytes{8}), 4, 2, 30).size() == 2);
}

// The bindings' concurrency: several threads each run pool jobs (overlapping: the persistent workers help
// whichever job has items left) and submit dispatcher tasks that themselves run pool jobs and wait on a task
// submitted before them (the VrfJob::after / SignJob::after_vrf pattern).
static void test_pool(int t) {
  for (int rep = 0; rep < 4; ++rep) {
    const size_t n = 200 + 37 * size_t(t) + size_t(rep);
    std::vector<long long> out(n, 0);
    parallel_for(n, 4 + t % 3, [&](size_t i) { out[i] = (long long)(i * i) + t; });
    long long sum = 0;
    for (size_t i = 0; i < n; ++i) sum += out[i];
    long long want = 0;
    for (size_t i = 0; i < n; ++i) want += (long long)(i * i) + t;
    CHECK(sum == want);
  }
  std::promise<long long> first_p;
  std::shared_future<long long> first = first_p.get_future().share();
  std::promise<long long> second_p;
  std::future<long long> second = second_p.get_future();
  std::vector<long long> a(300, 0);
  dispatcher().submit([&] {
    parallel_for(a.size(), 3, [&](size_t i) { a[i] = (long long)i * 3; });
    long long s = 0;
    for (long long v : a) s += v;
    first_p.set_value(s);
  });
  dispatcher().submit([&, first] {
    const long long f = first.get();   // runs once the earlier task is done
    second_p.set_value(f + a[299]);
  });
  const long long got = second.get();
  CHECK(got == 3ll * 299 * 300 / 2 + 3ll * 299);
  CHECK(first.get() == 3ll * 299 * 300 / 2);
}

// The share MSM's lane map (kernels/msm_lanes.h), exhaustively: over every lane of the grid the kernel is
// launched with, the lanes below neff * nchunks * SL hit every (pos, k, slot) exactly once and every other lane
// reports `none` -- for the plain and the grouped order, a short last group, a list compacted to fewer rows than
// the grid was sized for, and an empty list.
static void test_share_lanes() {
  for (int grid = 1; grid <= 130; ++grid) {
    std::vector<char> seen(size_t(grid), 0);
    for (int b = 0; b < grid; ++b) {
      const int l = xcd_remap(b, grid);
      CHECK(l >= 0 && l < grid && !seen[size_t(l)]);
      if (l >= 0 && l < grid) seen[size_t(l)] = 1;
    }
  }
  const int shapes[5][2] = {{70, 11}, {37, 6}, {248, 3}, {9, 30}, {1, 1}};
  for (const auto& sh : shapes) {
    const int nrows = sh[0], nchunks = sh[1];
    for (int SL : {1, 21, 22}) {
      const int grid = int(((long long)nrows * nchunks * SL + SHARE_MSM_THREADS - 1) / SHARE_MSM_THREADS);
      for (int group_rows : {0, 1, 8, 35, nrows + 5}) {
        for (int neff : {nrows, nrows - 3, 1, 0}) {
          if (neff < 0) continue;
          const long long total = (long long)neff * nchunks * SL;
          std::vector<char> seen(size_t(total), 0);
          long long hit = 0, bad = 0;
          for (int b = 0; b < grid; ++b)
            for (int t = 0; t < SHARE_MSM_THREADS; ++t) {
              const ShareLane l = share_lane(b, t, grid, neff, nchunks, SL, group_rows);
              if (l.none) continue;
              if (l.pos < 0 || l.pos >= neff || l.k < 0 || l.k >= nchunks || l.slot < 0 || l.slot >= SL) {
                ++bad;
                continue;
              }
              char& s = seen[(size_t(l.pos) * size_t(nchunks) + size_t(l.k)) * size_t(SL) + size_t(l.slot)];
              bad += s;
              s = 1;
              ++hit;
            }
          CHECK(bad == 0);
          CHECK(hit == total);   // with no repeats: every (pos, k, slot) once, every other lane `none`
        }
      }
    }
  }
}

// The fixed-base window plan (kernels/fixed_base.h): the entries of all (window, |digit|) tile [0, PB) exactly,
// and the signed-digit recoding rebuilds the scalar from digits inside each window's table.
static void test_fixed_base_plan() {
  const int plans[5][2] = {{8, 9}, {9, 8}, {11, 8}, {14, 8}, {8, 33}};   // NW = windows_for(B0); the Schnorr plan
  for (const auto& pl : plans) {
    const int B0 = pl[0], NW = pl[1];
    CHECK(fb_plan_ok(B0, NW));
    CHECK(fb_covers_i64(B0, NW));
    if (NW < 33) CHECK(NW == 1 + (65 - B0 + 7) / 8 && !fb_covers_i64(B0, NW - 1));
    const FbPlan p = fb_plan(B0, NW);
    CHECK(p.E0 == 1 << (B0 - 1) && p.PB == (long long)fb_runs(p) * FB_ENTRIES);
    std::vector<char> seen(size_t(p.PB), 0);
    long long n = 0;
    for (int w = 0; w < NW; ++w)
      for (int ad = 1; ad <= 1 << (fb_window_bits(p, w) - 1); ++ad, ++n) {
        const int e = fb_entry(p, w, ad);
        CHECK(e >= 0 && e < p.PB && !seen[size_t(e)]);
        if (e >= 0 && e < p.PB) seen[size_t(e)] = 1;
      }
    CHECK(n == p.PB);   // distinct and as many as the table has: [0, PB) exactly
    const long long half = 1ll << (B0 - 1);
    const long long cs[] = {0, 1, -1, half, -half, half + 1, -(half + 1), INT64_MAX, INT64_MIN};
    for (const long long c : cs) {
      // the primitives, as k_chunk_check uses them
      unsigned long long m = c < 0 ? 0ull - (unsigned long long)c : (unsigned long long)c;
      int carry = 0;
      __int128 sum = 0;
      for (int w = 0; w < NW; ++w) {
        const int bits = fb_window_bits(p, w);
        const int dg = fb_next_digit(m, carry, bits);
        CHECK(dg > -(1 << (bits - 1)) && dg <= 1 << (bits - 1));
        if (dg != 0) sum += (__int128)dg * ((__int128)1 << fb_window_shift(p, w));   // nonzero only below 2^72
      }
      CHECK(m == 0 && carry == 0);
      CHECK(sum == (c < 0 ? -(__int128)c : (__int128)c));
      // the walk, as the share and row MSMs use it
      __int128 walked = 0;
      fb_walk(c, p, [&](int w, int ad, bool negate) {
        CHECK(w >= 0 && w < NW && ad >= 1 && ad <= 1 << (fb_window_bits(p, w) - 1));
        const __int128 term = (__int128)ad << fb_window_shift(p, w);
        walked += negate ? -term : term;
      });
      CHECK(walked == (__int128)c);
    }
  }
  CHECK(!fb_plan_ok(7, 9) && !fb_plan_ok(21, 9) && !fb_plan_ok(8, 0) && !fb_covers_i64(14, 7));
}

int main(int argc, char** argv) {
  test_share_lanes();   // the kernels' host-checkable headers (pure functions), in either mode
  test_fixed_base_plan();
  if (argc > 1 && std::strcmp(argv[1], "pool") == 0) {
    // the concurrency stress alone (ThreadSanitizer runs: the crypto modules are ~10x slower under it)
    std::vector<std::thread> ts;
    for (int t = 0; t < 6; ++t) ts.emplace_back([t] { test_pool(t); test_hash(); test_protocol(); });
    for (auto& t : ts) t.join();
    std::printf("selftest pool: %s (%d failures)\n", failures ? "FAILED" : "ok", failures.load());
    return failures ? 1 : 0;
  }
  test_share_lanes();   // (repeated in the full run: milliseconds)
  test_fixed_base_plan();
  // run every module twice on 6 threads concurrently (lazy statics, caches and tables included)
  std::vector<std::thread> ts;
  for (int t = 0; t < 6; ++t)
    ts.emplace_back([t] {
      for (int r = 0; r < 2; ++r) {
        test_hash();
        test_curve();
        if (t < 2) test_pairing();
        test_vrf();
        test_shares_and_ledger();
        test_chain_audit_arrays();
        test_protocol();
        test_pool(t);
      }
    });
  for (auto& t : ts) t.join();
  std::printf("selftest: %s (%d failures)\n", failures ? "FAILED" : "ok", failures.load());
  return failures ? 1 : 0;
}
