// Queue + merge logic of the multi-problem launches (hrf_group.h); C-ABI: hrf_group_begin / hrf_group_end /
// hrf_group_count (include/hrfuser_hip.h).
#include <vector>
#include "hrf_group.h"
#include "../../include/hrfuser_hip.h"

namespace {
struct Pending {
  const void* kern;
  dim3 grid, block;
  unsigned smem, argsize;
  int call;
  hrf_grp_issue_t issue;
  size_t off;           // of the argument bytes in g_blob
};
thread_local bool g_on = false;
thread_local int g_call = -1;
thread_local int g_depth = 0;
thread_local std::vector<Pending> g_q;
thread_local std::vector<unsigned char> g_blob;
long g_count[3] = {0, 0, 0};   // launches issued by hrf_group_end, problems they carried, hrf_group_end calls

inline bool same(const Pending& a, const Pending& b) {
  return a.kern == b.kern && a.issue == b.issue && a.argsize == b.argsize && a.smem == b.smem &&
         a.grid.x == b.grid.x && a.grid.y == b.grid.y && a.grid.z == b.grid.z &&
         a.block.x == b.block.x && a.block.y == b.block.y && a.block.z == b.block.z;
}
}  // namespace

bool hrf_grp_collecting() { return g_on; }
void hrf_grp_enter() {
  if (g_depth++ == 0 && g_on) ++g_call;
}
void hrf_grp_leave() { --g_depth; }
void hrf_grp_push(const void* kern, dim3 grid, dim3 block, unsigned smem, const void* args, unsigned argsize,
                  hrf_grp_issue_t issue) {
  Pending p;
  p.kern = kern; p.grid = grid; p.block = block; p.smem = smem; p.argsize = argsize;
  p.call = g_call < 0 ? 0 : g_call;
  p.issue = issue;
  p.off = (g_blob.size() + 15) & ~(size_t)15;
  g_blob.resize(p.off + argsize);
  std::memcpy(g_blob.data() + p.off, args, argsize);
  g_q.push_back(p);
}

extern "C" int hrf_group_begin(void) {
  g_q.clear();
  g_blob.clear();
  g_call = -1;
  g_on = true;
  return HRF_OK;
}

extern "C" int hrf_group_end(void* stream) {
  g_on = false;
  ++g_count[2];
  const int n = (int)g_q.size();
  if (n == 0) return HRF_OK;
  const int ncalls = g_q.back().call + 1;
  std::vector<std::vector<int>> calls(ncalls);
  size_t maxlen = 0;
  for (int i = 0; i < n; ++i) {
    calls[g_q[i].call].push_back(i);
    maxlen = calls[g_q[i].call].size() > maxlen ? calls[g_q[i].call].size() : maxlen;
  }
  std::vector<char> done(n, 0);
  int rc = HRF_OK;
  // position k of every call, in call order: the launches of ONE call keep their order; launches of different calls are
  // independent by contract and merge when kernel instantiation and launch geometry are identical
  for (size_t k = 0; k < maxlen; ++k) {
    for (int c = 0; c < ncalls; ++c) {
      if (calls[c].size() <= k || done[calls[c][k]]) continue;
      const int i = calls[c][k];
      const unsigned char* argv[HRF_GROUP_MAX];
      int m = 0;
      argv[m++] = g_blob.data() + g_q[i].off;
      done[i] = 1;
      if (g_q[i].grid.z == 1) {
        for (int c2 = c + 1; c2 < ncalls && m < HRF_GROUP_MAX; ++c2) {
          if (calls[c2].size() <= k) continue;
          const int j = calls[c2][k];
          if (done[j] || !same(g_q[i], g_q[j])) continue;
          argv[m++] = g_blob.data() + g_q[j].off;
          done[j] = 1;
        }
      }
      const int r = g_q[i].issue(g_q[i].kern, g_q[i].grid, g_q[i].block, g_q[i].smem, stream, argv, m);
      if (r != HRF_OK) rc = r;
      ++g_count[0];
      g_count[1] += m;
    }
  }
  g_q.clear();
  g_blob.clear();
  return rc;
}

extern "C" long hrf_group_count(int what) {
  if (what == 3) return HRF_GROUP_MAX;                 // problems per launch this library was compiled for (1: pass-through)
  return (what >= 0 && what < 3) ? g_count[what] : -1;
}

// ---------------------------------------------------------------------------------------------- deterministic mode
// (include/hrfuser_hip.h: hrf_set_deterministic).  The mode is process-wide host state that every entry point reads when it
// ISSUES a launch (hrf_det_tag / hrf_det_grad in hrf_common.h put it into the launch's pointer arguments), so a
// captured graph replays the mode it was captured in.  Shadow bins of the fp32 gradient accumulators: a small table of
// registered ranges, looked up on the host per call.
#include <atomic>
#include <mutex>
#include "hrf_common.h"

namespace {
std::atomic<int> g_det{0};
struct DetRange { float* base; long n; long long* bins; };
constexpr int DET_MAX_RANGES = 64;
DetRange g_det_ranges[DET_MAX_RANGES];
int g_det_nranges = 0;
std::mutex g_det_mu;

// the registered range that holds [p, p + n)
bool det_find(const float* p, long n, DetRange& out) {
  std::lock_guard<std::mutex> lk(g_det_mu);
  for (int i = 0; i < g_det_nranges; ++i) {
    const DetRange& r = g_det_ranges[i];
    if (p >= r.base && p + n <= r.base + r.n) { out = r; return true; }
  }
  return false;
}

// g[i] += value(bins of i) where any bin is set, and the bins return to zero: ready for the next step without a memset
__global__ __launch_bounds__(256) void det_resolve_kernel(float* g, long long* bins, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    long long* b = bins + HRF_DET_BINS * i;
    const long long b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    if ((b0 | b1 | b2 | b3) != 0) {
      g[i] += (float)hrf_det_value(b0, b1, b2, b3);
      b[0] = 0; b[1] = 0; b[2] = 0; b[3] = 0;
    }
  }
}
}  // namespace

int hrf_det_on() { return g_det.load(std::memory_order_relaxed); }

float* hrf_det_grad(float* g, bool& ok) {
  if (g == nullptr || !hrf_det_on()) return g;
  DetRange r;
  if (!det_find(g, 1, r)) { ok = false; return nullptr; }
  return reinterpret_cast<float*>(reinterpret_cast<unsigned long long>(r.bins + HRF_DET_BINS * (g - r.base)) | 1ull);
}

extern "C" int hrf_set_deterministic(int on) {
  if (on && HRF_STAT_COPIES < HRF_DET_BINS) return HRF_ERR_ARG;   // the moment bins are the copies of a slot
  g_det.store(on ? 1 : 0, std::memory_order_relaxed);
  return HRF_OK;
}
extern "C" int hrf_get_deterministic(void) { return hrf_det_on(); }

extern "C" long hrf_det_bins_bytes(long n) { return n > 0 ? (long)(HRF_DET_BINS * sizeof(long long)) * n : 0; }

extern "C" int hrf_det_register(float* base, long n, void* bins) {
  if (base == nullptr || n <= 0 || (reinterpret_cast<unsigned long long>(bins) & 7ull) != 0) return HRF_ERR_ARG;
  std::lock_guard<std::mutex> lk(g_det_mu);
  int w = 0;
  for (int i = 0; i < g_det_nranges; ++i)                         // drop what the new range overlaps (re-allocated arenas)
    if (!(base + n <= g_det_ranges[i].base || g_det_ranges[i].base + g_det_ranges[i].n <= base)) continue;
    else g_det_ranges[w++] = g_det_ranges[i];
  g_det_nranges = w;
  if (bins == nullptr) return HRF_OK;
  if (g_det_nranges == DET_MAX_RANGES) return HRF_ERR_ARG;
  g_det_ranges[g_det_nranges++] = DetRange{base, n, static_cast<long long*>(bins)};
  return HRF_OK;
}

extern "C" int hrf_det_resolve(float* g, long n, void* stream) {
  if (g == nullptr || n < 0) return HRF_ERR_ARG;
  if (n == 0) return HRF_OK;
  DetRange r;
  if (!det_find(g, n, r)) return HRF_ERR_ARG;
  long nb = (n + 255) / 256;
  if (nb > 2048) nb = 2048;
  HRF_LAUNCH(det_resolve_kernel, dim3((unsigned)nb), dim3(256), 0, stream, g, r.bins + HRF_DET_BINS * (g - r.base), n);
  return hrf_check_launch();
}
