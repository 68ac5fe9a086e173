// pencil_stamps.hpp -- the cycle-stamp reports of the Gram walks (-DIGX_DEBUG, IGX_DEBUG_TIMING=n: the n-th launch of a launcher is the
// one that is stamped; diagnostic only).  The launchers (pencil_launch.hpp) ask a StampGate whether this launch is due, hand the kernel a
// zeroed buffer, and pass what it wrote to the report of their walk.  The per-CU timeline is gathered and summed up once, for the pencil walk and
// the two patch walks.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>
#include "gram_mfma.hpp"

namespace igx {

// one per launcher (a static of it): IGX_DEBUG_TIMING=n stamps the n-th launch of the process that the launcher makes (1: the first)
struct StampGate {
  int done = 0, seen = 0;
  bool due(const Space &s) {
    if (!(kDebug && s.env.debug_timing && !done && ++seen >= std::max(1, atoi(getenv("IGX_DEBUG_TIMING") ? getenv("IGX_DEBUG_TIMING") : "1")))) return false;
    done = 1;
    return true;
  }
};
static inline void stamps_alloc(PencilArgs &pa, size_t n) { (void)hipMalloc((void **)&pa.debug_buf, n * 8); (void)hipMemset(pa.debug_buf, 0, n * 8); }
static inline std::vector<long long> stamps_fetch(hipStream_t stream, PencilArgs &pa, size_t n) {
  (void)hipStreamSynchronize(stream);
  std::vector<long long> h(n);
  (void)hipMemcpy(h.data(), pa.debug_buf, n * 8, hipMemcpyDeviceToHost);
  (void)hipFree(pa.debug_buf); pa.debug_buf = nullptr;
  return h;
}

// The launch as a timeline on the 100 MHz clock the XCCs share: per CU (XCC, SE, SH, CU of HW_ID) the workgroups' {entry, exit} from
// their records wr[workgroup][4] = {entry, exit, HW_ID, XCC_ID}, the launch's first entry t0 and last exit t1.
struct CuTimeline {
  long long t0 = LLONG_MAX, t1 = 0;
  std::map<long long, std::vector<std::pair<long long, long long>>> cu;
  bool any() const { return t1 > t0 && !cu.empty(); }
};
static inline CuTimeline cu_timeline(const long long *wr, size_t nwg) {
  CuTimeline T;
  for (size_t b = 0; b < nwg; ++b) {
    const long long *w = wr + b * 4;
    if (!w[0] || !w[1]) continue;
    T.t0 = std::min(T.t0, w[0]); T.t1 = std::max(T.t1, w[1]);
    const long long hw = w[2], key = ((w[3] & 15) << 12) | (((hw >> 13) & 7) << 8) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15);
    T.cu[key].push_back({w[0], w[1]});
  }
  return T;
}

// where the time between the first entry and the last exit goes: per CU the workgroups in the order they ran, how late the first
// one starts (dispatch ramp), the gap between one workgroup's exit and the next one's entry, the tail after its last exit
static void report_cu_timeline(const char *tag, CuTimeline &T) {
  if (!T.any()) return;
  const long long t0 = T.t0, t1 = T.t1;
  const double span = (double)(t1 - t0);
  double busy = 0, ramp = 0, gap = 0, tail = 0, life1 = 0, life2 = 0, ramp_max = 0; long long n1 = 0, n2 = 0, ngap = 0; int rounds_max = 0;
  for (auto &kv : T.cu) {
    auto &v = kv.second; std::sort(v.begin(), v.end());
    ramp += (double)(v.front().first - t0); ramp_max = std::max(ramp_max, (double)(v.front().first - t0));
    tail += (double)(t1 - v.back().second);
    rounds_max = std::max(rounds_max, (int)v.size());
    for (size_t i = 0; i < v.size(); ++i) {
      busy += (double)(v[i].second - v[i].first);
      if (i == 0) { life1 += (double)(v[i].second - v[i].first); n1++; } else { life2 += (double)(v[i].second - v[i].first); n2++; gap += (double)(v[i].first - v[i - 1].second); ngap++; }
    }
  }
  const double ncu = (double)T.cu.size();
  fprintf(stderr, "%s   timeline (100 MHz ticks = 10 ns): span %.0f = %.1f us over %d CUs that ran a workgroup, at most %d workgroups on one CU\n", tag, span, span * 0.01, (int)T.cu.size(), rounds_max);
  fprintf(stderr, "%s   per CU, mean ticks: first entry after the launch's first %.0f (max %.0f) | busy %.0f | between workgroups %.1f (x %.2f per CU) | idle after its last exit %.0f\n",
          tag, ramp / ncu, ramp_max, busy / ncu, ngap ? gap / ngap : 0.0, (double)ngap / ncu, tail / ncu);
  fprintf(stderr, "%s   workgroup life, ticks: first on its CU %.0f (%lld) | later ones %.0f (%lld); CU-time in a workgroup's life %.3f of span x CUs (x %.3f of 256 CUs)\n",
          tag, n1 ? life1 / n1 : 0.0, n1, n2 ? life2 / n2 : 0.0, n2, busy / (span * ncu), busy / (span * 256.0));
  // ... and per XCC (the key's bits 12-15): its CUs and workgroups, the mean and the extremes of a workgroup's life, when its CUs
  // leave their last workgroup as a share of the span -- a launch waits for its slowest XCC
  struct Xcc { int cus = 0; long long n = 0; double life = 0, lmin = 1e30, lmax = 0, last = 0, last_min = 1e30, last_max = 0; };
  std::map<long long, Xcc> xc;
  for (auto &kv : T.cu) {
    Xcc &x = xc[kv.first >> 12];
    x.cus++;
    for (auto &iv : kv.second) { const double l = (double)(iv.second - iv.first); x.n++; x.life += l; x.lmin = std::min(x.lmin, l); x.lmax = std::max(x.lmax, l); }
    const double e = (double)(kv.second.back().second - t0) / span;
    x.last += e; x.last_min = std::min(x.last_min, e); x.last_max = std::max(x.last_max, e);
  }
  for (auto &kv : xc) {
    const Xcc &x = kv.second;
    fprintf(stderr, "%s   XCC %lld: %d CUs, %lld workgroups, life mean %.0f (min %.0f, max %.0f) ticks; last exit of a CU at %.3f of the span (min %.3f, max %.3f)\n",
            tag, kv.first, x.cus, x.n, x.life / x.n, x.lmin, x.lmax, x.last / x.cus, x.last_min, x.last_max);
  }
}

// gram_pencil_body's stamps: [workgroup][2 waves][64 entries][4] phase stamps, then the workgroups' records
static inline size_t pencil_stamp_count(const PencilArgs &pa) { const size_t nwg = (size_t)pa.blocks_per_seg * pa.nseg; return nwg * 2 * 64 * 4 + nwg * 4; }
static void report_pencil_stamps(const std::vector<long long> &h, const PencilArgs &pa) {
  const size_t dbg_blocks = (size_t)pa.blocks_per_seg * pa.nseg;
  double sm = 0, sw = 0, sf = 0, sp = 0; long long cnt = 0; long long hist[16] = {0};
  for (size_t b = 0; b < dbg_blocks * 2; ++b) for (int e = 4; e < 60; ++e) {
    const long long *d = &h[(b * 64 + e) * 4], *dn = &h[(b * 64 + e + 1) * 4];
    if (!d[3] || !dn[0]) continue;
    sm += (double)(d[1] - d[0]); sw += (double)(d[2] - d[1]); sf += (double)(d[3] - d[2]); sp += (double)(dn[0] - d[0]); cnt++;
    long long fb = (d[3] - d[2]) / 8192; if (fb > 15) fb = 15; hist[fb]++;
  }
  fprintf(stderr, "[igx pencil timing] blocks=%d seg_len=%d n=%lld cycles: mfma %.0f | wait@barrier %.0f | flush %.0f | period %.0f\n   flush histogram (8192-cycle bins):",
          pa.blocks_per_seg * pa.nseg, pa.seg_len, cnt, sm / cnt, sw / cnt, sf / cnt, sp / cnt);
  for (int i = 0; i < 16; ++i) fprintf(stderr, " %lld", hist[i]);
  fprintf(stderr, "\n");
  {   // the life of a workgroup (wave 0): entry -> tables staged -> first element -> last element -> end
    double a = 0, b2 = 0, c = 0, d2 = 0, nel = 0; long long nb = 0;
    for (size_t b = 0; b < dbg_blocks; ++b) {
      const long long *d = &h[((b * 2) * 64 + 62) * 4];
      if (!d[0] || !d[4]) continue;
      a += (double)(d[1] - d[0]); b2 += (double)(d[2] - d[1]); c += (double)(d[3] - d[2]); d2 += (double)(d[4] - d[3]); nel += (double)d[5]; nb++;
    }
    if (nb) fprintf(stderr, "[igx pencil timing] workgroup life (wave 0, mean of %lld): staging %.0f | lane set-up %.0f | walk %.0f (%.1f elements) | trailing leaves %.0f cycles\n", nb, a / nb, b2 / nb, c / nb, nel / nb, d2 / nb);
    // ... its spread, per segment of the pencils, and the span of the launch (first entry to last end) on the same counter
    for (int sg = 0; sg < pa.nseg; ++sg) {
      double mn = 1e30, mx = 0, sm2 = 0; long long n2 = 0;
      for (int bb = 0; bb < pa.blocks_per_seg; ++bb) {
        const long long *d = &h[(((size_t)sg * pa.blocks_per_seg + bb) * 2 * 64 + 62) * 4];
        if (!d[0] || !d[4]) continue;
        const double life = (double)(d[4] - d[0]); mn = std::min(mn, life); mx = std::max(mx, life); sm2 += life; n2++;
      }
      if (n2) fprintf(stderr, "[igx pencil timing]   segment %d: %lld workgroups, life min %.0f mean %.0f max %.0f\n", sg, n2, mn, sm2 / n2, mx);
    }
  }
  CuTimeline T = cu_timeline(&h[dbg_blocks * 2 * 64 * 4], dbg_blocks);
  report_cu_timeline("[igx pencil timing]", T);
}

// gram_patch_p2's stamps: [workgroup][W wavefronts][4] = cycles in three phases and the elements walked, then the workgroups' records
static inline size_t patch2_stamp_count(const PencilArgs &pa, int W) { const size_t nwg = (size_t)pa.blocks_per_seg * pa.nseg; return nwg * W * 4 + nwg * 4; }
static void report_patch2_stamps(const std::vector<long long> &h, const PencilArgs &pa, int W, int cx, int cy) {
  const size_t nwg = (size_t)pa.blocks_per_seg * pa.nseg;
  double sm[3][3] = {{0}}; long long cnt[3] = {0}; double el = 0;
  for (size_t b = 0; b < nwg; ++b) for (int w = 0; w < W; ++w) {
    const long long *d = &h[(b * W + w) * 4];
    if (!d[3]) continue;
    const int k = w < 7 ? 0 : (w < W - 1 ? 1 : 2);      // wavefronts whose every lane owns a run | partly or none | the one with the F rows
    for (int c = 0; c < 3; ++c) sm[k][c] += (double)d[c] / (double)d[3];
    cnt[k]++; el += (double)d[3];
  }
  const char *nm[3] = {"wavefronts 0-6 (64 runs each)", "wavefronts 7-10 (8 runs / none)", "wavefront 11 (the F rows)"};
  fprintf(stderr, "[igx patch timing] colour (%d,%d): %zu workgroups, seg_len %d nseg %d; cycles per element and wavefront:\n", cx, cy, nwg, pa.seg_len, pa.nseg);
  for (int k = 0; k < 3; ++k) if (cnt[k]) fprintf(stderr, "[igx patch timing]   %s: MFMAs + window adds %.0f | wait at the barrier %.0f | leave + next fetch %.0f | period %.0f\n", nm[k], sm[k][0] / cnt[k], sm[k][1] / cnt[k], sm[k][2] / cnt[k], (sm[k][0] + sm[k][1] + sm[k][2]) / cnt[k]);
  const CuTimeline T = cu_timeline(&h[nwg * W * 4], nwg);
  if (!T.any()) return;
  double busy = 0; int rmax = 0;
  for (auto &kv : T.cu) { rmax = std::max(rmax, (int)kv.second.size()); for (auto &iv : kv.second) busy += (double)(iv.second - iv.first); }
  fprintf(stderr, "[igx patch timing]   timeline: span %.1f us (walks only) over %d CUs, at most %d workgroups on one CU; CU-time inside a walk %.3f of span x 256 CUs\n",
          (T.t1 - T.t0) * 0.01, (int)T.cu.size(), rmax, busy / ((double)(T.t1 - T.t0) * 256.0));
}

// gram_pencil_patch3's stamps: [workgroup][W wavefronts][8] = cycles in five parts of a step, the element steps, and on the 100 MHz clock
// the set-up before the walk and the trailing layers behind it; then the workgroups' records
static inline size_t patch3_stamp_count(const PencilArgs &pa, int W) { const size_t nwg = (size_t)pa.blocks_per_seg * pa.nseg; return nwg * W * 8 + nwg * 4; }
static void report_patch3_stamps(const std::vector<long long> &h, const PencilArgs &pa, int W, int cx, int cy) {
  const size_t nwg = (size_t)pa.blocks_per_seg * pa.nseg;
  double sm[5] = {0, 0, 0, 0, 0}, mx[5] = {0, 0, 0, 0, 0}, steps = 0, setup = 0, trail = 0; long long cnt = 0;
  for (size_t i = 0; i < nwg * W; ++i) {
    const long long *d = &h[i * 8];
    if (!d[5]) continue;
    for (int c = 0; c < 5; ++c) { const double x = (double)d[c] / (double)d[5]; sm[c] += x; mx[c] = std::max(mx[c], x); }
    cnt++;
    if (i % W == 0) { steps += (double)d[5]; setup += (double)d[6]; trail += (double)d[7]; }
  }
  if (cnt) fprintf(stderr, "[igx patch3 timing] colour (%d,%d): %zu workgroups, seg_len %d nseg %d; cycles per element step, mean (max) over %lld wavefronts: products %.0f (%.0f) | ticks %.0f (%.0f) | wait for the old values %.0f (%.0f) | window, stores, next loads %.0f (%.0f) | closing barrier + F %.0f (%.0f) | step %.0f\n",
                   cx, cy, nwg, pa.seg_len, pa.nseg, cnt, sm[0] / cnt, mx[0], sm[1] / cnt, mx[1], sm[2] / cnt, mx[2], sm[3] / cnt, mx[3], sm[4] / cnt, mx[4], (sm[0] + sm[1] + sm[2] + sm[3] + sm[4]) / cnt);
  CuTimeline T = cu_timeline(&h[nwg * W * 8], nwg);
  if (!T.any()) return;
  report_cu_timeline("[igx patch3 timing]", T);
  // the launch's CU-time outside the element steps: set-up and trailing layers inside a workgroup's life, the rest of the span outside it
  double busy = 0;
  for (auto &kv : T.cu) for (auto &iv : kv.second) busy += (double)(iv.second - iv.first);
  const double span = (double)(T.t1 - T.t0), walk = busy - setup - trail;
  fprintf(stderr, "[igx patch3 timing]   %.0f element steps in all, %.1f per CU of 256; of span x 256 CUs: inside a walk's steps %.3f | set-up before the walk %.3f | trailing layers %.3f | no workgroup on the CU %.3f; ticks per step inside a walk %.2f\n",
          steps, steps / 256.0, walk / (span * 256.0), setup / (span * 256.0), trail / (span * 256.0), 1.0 - busy / (span * 256.0), steps ? walk / steps : 0.0);
}

}  // namespace igx
