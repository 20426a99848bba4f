// tfimm_hip_knn_vote / tfimm_hip_knn_score: the k matches of a gallery search (tfimm_hip_embed_search's indices and scores)
// turned into classes through the gallery's label table -- a weighted vote or the best row per identity -- and, for a labelled
// batch, scored into the accumulators of tfimm_hip_score (include/tfimm_hip.h; the CPU restatement of the
// rule is tests/knn_ref.py).  Replaces, in a caller of the search: the (B, k) indices copied to the host, the label lookup,
// the vote and the accuracy counters there.
//
// One wave per query, four queries per workgroup (the mapping of l2_normalize in embed.hip); lane j owns candidate j, k <= 64.
//   1. lane j reads indices[j], scores[j] and -- only for an index inside [0, N) that is not the excluded row -- the row's
//      label.  A candidate that is not valid carries the label -1 and the weight 0 from here on.
//   2. SUM: m = the largest valid score (a butterfly of maxima: exact, every lane holds the same bits),
//      w_j = expf((s_j - m) * inv_temperature): one subtraction, one product, expf.
//   3. a uniform loop over i = 0 .. k-1 broadcasts lane i's label and weight (v_readlane: the loop counter is scalar); the
//      lanes that hold the same label add.  Every lane of a class thus forms the class sum in ascending candidate order, from
//      the same operands: the same bits in all of them, whatever B.  The lowest lane of a class is its leader.
//   4. a second uniform loop over the leaders (the set bits of one ballot) counts, per leader, the leaders that beat it -- a
//      larger value, or an equal value and a lower class: its position in the list.
//   5. vote: a leader whose position is below `top` writes its slot, the lanes [distinct, top) write the empty slots.
//      score: the true class's rank among nb_classes is counted from ballots over the leaders alone (the unvoted classes
//      all hold 0: those below y beat it exactly when v[y] == 0, and there are y - |voted classes below y| of them); lane 0
//      writes the four outputs and issues the integer atomics of the meter.
// Registers and cross-lane operations only: no LDS, no barrier, no float atomics, no allocation; rows never mix.
#include "common.h"

// w_j is the product rounded, then expf; nothing here may contract
#pragma clang fp contract(off)

namespace {

constexpr int kRows = 4;   // queries (= waves) per workgroup

struct KnnArgs {
  const int32_t* indices;
  const uint32_t* scores;   // float32 bits
  const int32_t* glabels;
  const int32_t* exclude;   // or null
  int64_t ld;
  int B, k, N;
  int label_end;            // a label votes when it is in [0, label_end): INT32_MAX in the vote ("any non-negative label" is
                            // [0, INT32_MAX] there, tested as >= 0 alone), nb_classes in the scoring entry point
  float inv_t;
  int reduce, top;
  // vote
  int32_t* classes;
  float* values;
  int32_t* counts;
  float* total;
  // score
  const int32_t* labels;
  float* loss;
  int32_t* rank;
  int32_t* pred;
  float* prob;
  unsigned long long* state;
  unsigned long long* per_class;
  uint32_t* confusion;
};

__device__ __forceinline__ int lane_int(int v, int i) { return __builtin_amdgcn_readlane(v, i); }
__device__ __forceinline__ float lane_float(float v, int i) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// What one query's candidates vote: per lane its class's value and count, whether it leads its class, and its position.
struct Vote {
  int lab;                       // this lane's class, -1: the candidate is not valid
  float value;                   // its class's value (every lane of a class holds the same bits)
  int count;
  bool leader;
  unsigned long long leaders;    // ballot of `leader`
  int pos;                       // leaders only: how many leaders beat this one
  float total;
};

template <bool kScore>
__device__ __forceinline__ Vote vote_row(const KnnArgs& a, int64_t row, int lane) {
  const int k = a.k;
  Vote v;
  // ---- 1. the candidate.  Columns >= k are never read; no label is read for an index outside [0, N)
  int lab = -1;
  float s = 0.f;
  if (lane < k) {
    const int idx = a.indices[row * a.ld + lane];
    const int ex = a.exclude ? a.exclude[row] : -1;
    if (idx >= 0 && idx < a.N && idx != ex) {
      lab = a.glabels[idx];
      if (kScore && lab >= a.label_end) lab = -1;
      if (lab < 0) lab = -1;
      s = __uint_as_float(a.scores[row * a.ld + lane]);
    }
  }
  const bool valid = lab >= 0;
  const bool sum = kScore || a.reduce == TFIMM_KNN_SUM;

  // ---- 2. the weight
  float w = s;
  if (sum) {
    const float m = wave_max(valid ? s : -INFINITY);
    w = valid ? expf((s - m) * a.inv_t) : 0.f;
  }

  // ---- 3. per class: value and count in ascending candidate order; the lowest lane of a class leads it
  float value = 0.f, total = 0.f;
  int count = 0;
  bool leader = valid;
  for (int i = 0; i < k; ++i) {
    const int li = lane_int(lab, i);
    const float wi = lane_float(w, i);
    if (li < 0) continue;                              // uniform
    const bool mine = li == lab;
    if (sum) {
      total += wi;
      if (mine) value += wi;
    } else if (mine && (count == 0 || wi > value)) {   // among equal maxima the first stays: -0.0 > +0.0 is false
      value = wi;
    }
    if (mine) {
      ++count;
      if (i < lane) leader = false;
    }
  }
  const unsigned long long leaders = __ballot(leader);

  // ---- 4. a leader's position: the leaders that beat it
  int pos = 0;
  for (unsigned long long rest = leaders; rest; rest &= rest - 1) {
    const int i = (int)__builtin_ctzll(rest);          // scalar: the ballot is
    const int li = lane_int(lab, i);
    const float vi = lane_float(value, i);
    pos += (vi > value || (vi == value && li < lab)) ? 1 : 0;
  }
  v.lab = lab;
  v.value = value;
  v.count = count;
  v.leader = leader;
  v.leaders = leaders;
  v.pos = pos;
  v.total = total;
  return v;
}

__global__ void __launch_bounds__(64 * kRows) knn_vote_kernel(KnnArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kRows + (threadIdx.x >> 6);
  if (row >= a.B) return;
  const Vote v = vote_row<false>(a, row, lane);
  const int top = a.top;
  const int64_t out = row * top;
  if (v.leader && v.pos < top) {
    a.classes[out + v.pos] = v.lab;
    a.values[out + v.pos] = v.value;
    a.counts[out + v.pos] = v.count;
  }
  const int distinct = __popcll(v.leaders);
  if (lane >= distinct && lane < top) {                // top <= 64: one lane per empty slot
    a.classes[out + lane] = -1;
    a.values[out + lane] = 0.f;
    a.counts[out + lane] = 0;
  }
  if (lane == 0) a.total[row] = v.total;               // MAX: never added to, +0.0
}

__global__ void __launch_bounds__(64 * kRows) knn_score_kernel(KnnArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kRows + (threadIdx.x >> 6);
  if (row >= a.B) return;
  const Vote v = vote_row<true>(a, row, lane);
  const int C = a.label_end;
  const int y = a.labels[row];
  const bool scored = y >= 0 && y < C;

  // pred: the leader nothing beats.  Any valid candidate makes the largest score's class hold a weight of expf(0) = 1, above
  // the 0 of every unvoted class; with none, every class holds 0 and class 0 is first
  const unsigned long long first = __ballot(v.leader && v.pos == 0);
  const int pred = first ? __shfl(v.lab, (int)__builtin_ctzll(first), 64) : 0;

  // the true class's value: its leader's, or the 0 of an unvoted class
  const unsigned long long own = __ballot(v.leader && v.lab == y);
  const float vy = (scored && own) ? __shfl(v.value, (int)__builtin_ctzll(own), 64) : 0.f;
  // rank: voted classes that beat y, and -- when v[y] == 0 -- the unvoted classes below y, which tie with it.  A voted class
  // below y whose value is exactly 0 is among the first and, being voted, not among the second
  const int beat = __popcll(__ballot(v.leader && v.lab != y && (v.value > vy || (v.value == vy && v.lab < y))));
  const int below = __popcll(__ballot(v.leader && v.lab < y));
  if (lane != 0) return;

  float loss = 0.f, prob = 0.f;
  int rank = y == TFIMM_SCORE_IGNORE ? -1 : -2;
  if (scored) {
    rank = beat + (vy == 0.f ? y - below : 0);
    prob = v.total == 0.f ? 0.f : __fdiv_rn(vy, v.total);
    loss = 0.f - logf(prob);
  }
  a.loss[row] = loss;
  a.rank[row] = rank;
  a.pred[row] = pred;
  a.prob[row] = prob;

  // ---- the meter: tfimm_hip_score's, statement for statement
  if (a.state != nullptr) {
    if (!scored) {
      atomicAdd(a.state + (y == TFIMM_SCORE_IGNORE ? TFIMM_SCORE_IGNORED : TFIMM_SCORE_INVALID), 1ull);
    } else {
      atomicAdd(a.state + TFIMM_SCORE_SCORED, 1ull);
      if (loss < 1024.0f)   // false for a NaN and for the +inf of a true class nobody voted for
        atomicAdd(a.state + TFIMM_SCORE_LOSS_Q, (unsigned long long)__double2ll_rn((double)loss * 4294967296.0));
      else
        atomicAdd(a.state + TFIMM_SCORE_LOSS_EXCLUDED, 1ull);
      atomicAdd(a.state + TFIMM_SCORE_RANK_HIST + min(rank, TFIMM_SCORE_RANK_BINS - 1), 1ull);
    }
  }
  if (scored && a.per_class != nullptr) {
    atomicAdd(a.per_class + y, 1ull);
    if (rank == 0) atomicAdd(a.per_class + C + y, 1ull);
  }
  if (scored && a.confusion != nullptr)   // pred is a voting label, below nb_classes, or 0
    atomicAdd(a.confusion + (int64_t)y * C + pred, 1u);
}

// what both entry points refuse alike; `who` starts every message
int check_common(const char* who, const int32_t* indices, const float* scores, int64_t ld, int B, int k, const int32_t* glabels,
                 int N, const int32_t* exclude, float inv_temperature) {
  if (!indices) TFIMM_FAIL(TFIMM_EINVAL, "%s: indices is null", who);
  if (!scores) TFIMM_FAIL(TFIMM_EINVAL, "%s: scores is null", who);
  if (!glabels) TFIMM_FAIL(TFIMM_EINVAL, "%s: glabels is null", who);
  if (((uintptr_t)indices | (uintptr_t)scores | (uintptr_t)glabels | (uintptr_t)exclude) & 3)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: indices, scores, glabels and exclude hold 4-byte elements and must be 4-byte aligned", who);
  if (k < 1 || k > TFIMM_KNN_MAX_K) TFIMM_FAIL(TFIMM_EINVAL, "%s: k=%d, must be in [1, TFIMM_KNN_MAX_K = %d]", who, k, TFIMM_KNN_MAX_K);
  if (ld < k) TFIMM_FAIL(TFIMM_EINVAL, "%s: ld=%lld is smaller than k=%d", who, (long long)ld, k);
  if (N < 1) TFIMM_FAIL(TFIMM_EINVAL, "%s: N=%d, must be at least 1", who, N);
  if (B < 0) TFIMM_FAIL(TFIMM_EINVAL, "%s: B=%d is negative", who, B);
  if (!(inv_temperature >= 0.f) || inv_temperature > 3.402823466e38f)   // a NaN fails the first comparison
    TFIMM_FAIL(TFIMM_EINVAL, "%s: inv_temperature=%g, must be finite and not negative", who, (double)inv_temperature);
  return 0;
}

}  // namespace

extern "C" int tfimm_hip_knn_vote(const int32_t* indices, const float* scores, int64_t ld, int B, int k, const int32_t* glabels,
                                  int N, const int32_t* exclude, float inv_temperature, int reduce, int top, int32_t* classes,
                                  float* values, int32_t* counts, float* total, void* stream) {
  if (int rc = check_common("knn_vote", indices, scores, ld, B, k, glabels, N, exclude, inv_temperature)) return rc;
  if (!classes) TFIMM_FAIL(TFIMM_EINVAL, "knn_vote: classes is null");
  if (!values) TFIMM_FAIL(TFIMM_EINVAL, "knn_vote: values is null");
  if (!counts) TFIMM_FAIL(TFIMM_EINVAL, "knn_vote: counts is null");
  if (!total) TFIMM_FAIL(TFIMM_EINVAL, "knn_vote: total is null");
  if (((uintptr_t)classes | (uintptr_t)values | (uintptr_t)counts | (uintptr_t)total) & 3)
    TFIMM_FAIL(TFIMM_EINVAL, "knn_vote: classes, values, counts and total hold 4-byte elements and must be 4-byte aligned");
  if (reduce != TFIMM_KNN_SUM && reduce != TFIMM_KNN_MAX)
    TFIMM_FAIL(TFIMM_EINVAL, "knn_vote: reduce=%d, must be TFIMM_KNN_SUM or TFIMM_KNN_MAX", reduce);
  if (top < 1 || top > TFIMM_KNN_MAX_TOP)
    TFIMM_FAIL(TFIMM_EINVAL, "knn_vote: top=%d, must be in [1, TFIMM_KNN_MAX_TOP = %d]", top, TFIMM_KNN_MAX_TOP);
  if (B == 0) return 0;
  KnnArgs a = {};
  a.indices = indices;
  a.scores = reinterpret_cast<const uint32_t*>(scores);
  a.glabels = glabels;
  a.exclude = exclude;
  a.ld = ld;
  a.B = B;
  a.k = k;
  a.N = N;
  a.label_end = INT32_MAX;
  a.inv_t = inv_temperature;
  a.reduce = reduce;
  a.top = top;
  a.classes = classes;
  a.values = values;
  a.counts = counts;
  a.total = total;
  const dim3 grid((unsigned)(((int64_t)B + kRows - 1) / kRows));
  TFIMM_LAUNCH(knn_vote_kernel, grid, dim3(64 * kRows), 0, (hipStream_t)stream, a);
  return 0;
}

extern "C" int tfimm_hip_knn_score(const int32_t* indices, const float* scores, int64_t ld, int B, int k, const int32_t* glabels,
                                   int N, const int32_t* exclude, float inv_temperature, int nb_classes, const int32_t* labels,
                                   float* loss, int32_t* rank, int32_t* pred, float* prob, int64_t* state, int64_t* per_class,
                                   uint32_t* confusion, void* stream) {
  if (int rc = check_common("knn_score", indices, scores, ld, B, k, glabels, N, exclude, inv_temperature)) return rc;
  if (!labels) TFIMM_FAIL(TFIMM_EINVAL, "knn_score: labels is null");
  if (!loss) TFIMM_FAIL(TFIMM_EINVAL, "knn_score: loss is null");
  if (!rank) TFIMM_FAIL(TFIMM_EINVAL, "knn_score: rank is null");
  if (!pred) TFIMM_FAIL(TFIMM_EINVAL, "knn_score: pred is null");
  if (!prob) TFIMM_FAIL(TFIMM_EINVAL, "knn_score: prob is null");
  if (((uintptr_t)labels | (uintptr_t)loss | (uintptr_t)rank | (uintptr_t)pred | (uintptr_t)prob | (uintptr_t)confusion) & 3)
    TFIMM_FAIL(TFIMM_EINVAL, "knn_score: labels, loss, rank, pred, prob and confusion hold 4-byte elements and must be 4-byte aligned");
  if (((uintptr_t)state | (uintptr_t)per_class) & 7)
    TFIMM_FAIL(TFIMM_EINVAL, "knn_score: state and per_class hold 8-byte elements and must be 8-byte aligned");
  if (nb_classes < 1) TFIMM_FAIL(TFIMM_EINVAL, "knn_score: nb_classes=%d, must be at least 1", nb_classes);
  if (confusion && nb_classes > TFIMM_SCORE_MAX_CONFUSION_N)
    TFIMM_FAIL(TFIMM_EINVAL, "knn_score: confusion with nb_classes=%d, more than TFIMM_SCORE_MAX_CONFUSION_N = %d", nb_classes,
               TFIMM_SCORE_MAX_CONFUSION_N);
  if (B == 0) return 0;
  KnnArgs a = {};
  a.indices = indices;
  a.scores = reinterpret_cast<const uint32_t*>(scores);
  a.glabels = glabels;
  a.exclude = exclude;
  a.ld = ld;
  a.B = B;
  a.k = k;
  a.N = N;
  a.label_end = nb_classes;
  a.inv_t = inv_temperature;
  a.reduce = TFIMM_KNN_SUM;
  a.labels = labels;
  a.loss = loss;
  a.rank = rank;
  a.pred = pred;
  a.prob = prob;
  a.state = reinterpret_cast<unsigned long long*>(state);
  a.per_class = reinterpret_cast<unsigned long long*>(per_class);
  a.confusion = confusion;
  const dim3 grid((unsigned)(((int64_t)B + kRows - 1) / kRows));
  TFIMM_LAUNCH(knn_score_kernel, grid, dim3(64 * kRows), 0, (hipStream_t)stream, a);
  return 0;
}
