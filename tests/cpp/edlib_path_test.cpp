// racon's alignment call against include/edlib.h (the drop-in served by libraven_hip.so):
//   edlibAlign(q, qlen, t, tlen, edlibNewAlignConfig(-1, EDLIB_MODE_NW, EDLIB_TASK_PATH, nullptr, 0))
//   -> result.alignment / alignmentLength -> edlibAlignmentToCigar -> edlibFreeAlignResult
// (Overlap::find_breaking_points, behind RavenLib/src/polish.cc:43-51), from 8 threads at once and mixed with the
// distance requests of construct.cc, so that both kinds meet in the combining queue.  Every PATH result is checked against
// a DP traceback computed here with the rule the header states: from the end, the diagonal, then 'I', then 'D'.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "edlib.h"

// distance and op string (one EDLIB_EDOP_* byte per column) of query against target
static int dp_path(const std::string& q, const std::string& t, std::vector<unsigned char>* ops) {
  const size_t n = t.size(), m = q.size(), m1 = m + 1;
  std::vector<int> D((n + 1) * m1);
  for (size_t j = 0; j <= m; ++j) D[j] = static_cast<int>(j);
  for (size_t i = 1; i <= n; ++i) {
    D[i * m1] = static_cast<int>(i);
    for (size_t j = 1; j <= m; ++j)
      D[i * m1 + j] = std::min(std::min(D[(i - 1) * m1 + j] + 1, D[i * m1 + j - 1] + 1), D[(i - 1) * m1 + j - 1] + (t[i - 1] != q[j - 1]));
  }
  ops->clear();
  size_t i = n, j = m;
  while (i > 0 || j > 0) {
    const int d = D[i * m1 + j];
    if (i > 0 && j > 0 && D[(i - 1) * m1 + j - 1] + (t[i - 1] != q[j - 1]) == d) {
      ops->push_back(t[i - 1] != q[j - 1] ? EDLIB_EDOP_MISMATCH : EDLIB_EDOP_MATCH);
      --i;
      --j;
    } else if (j > 0 && D[i * m1 + j - 1] + 1 == d) {
      ops->push_back(EDLIB_EDOP_INSERT);
      --j;
    } else {
      ops->push_back(EDLIB_EDOP_DELETE);
      --i;
    }
  }
  std::reverse(ops->begin(), ops->end());
  return D[n * m1 + m];
}

// 0 = the result is a valid alignment of cost editDistance = want, equal to the traceback; else which check failed
static int check_path(const EdlibAlignResult& r, const std::string& q, const std::string& t) {
  std::vector<unsigned char> want;
  const int d = dp_path(q, t, &want);
  if (r.status != EDLIB_STATUS_OK) return 1;
  if (r.editDistance != d) return 2;
  if (r.numLocations != 1 || !r.endLocations || r.endLocations[0] != static_cast<int>(t.size()) - 1 || !r.startLocations ||
      r.startLocations[0] != 0)
    return 3;
  if (r.alignmentLength < 0 || (r.alignmentLength > 0 && !r.alignment)) return 4;
  size_t qi = 0, ti = 0;
  int cost = 0;
  for (int x = 0; x < r.alignmentLength; ++x) {
    const unsigned char op = r.alignment[x];
    if (op > 3) return 5;  // ops valid
    if (op == EDLIB_EDOP_MATCH || op == EDLIB_EDOP_MISMATCH) {
      if (qi >= q.size() || ti >= t.size()) return 6;
      if ((q[qi] == t[ti]) != (op == EDLIB_EDOP_MATCH)) return 7;  // '=' / 'X' agree with the bytes
      ++qi;
      ++ti;
    } else if (op == EDLIB_EDOP_INSERT) {
      if (qi >= q.size()) return 6;
      ++qi;
    } else {
      if (ti >= t.size()) return 6;
      ++ti;
    }
    cost += op != EDLIB_EDOP_MATCH;
  }
  if (qi != q.size() || ti != t.size()) return 8;  // ops consume both strings
  if (cost != d) return 9;
  if (static_cast<size_t>(r.alignmentLength) != want.size() || (want.size() && std::memcmp(r.alignment, want.data(), want.size()) != 0))
    return 10;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::vector<std::string> seqs;
  std::string line;
  while (std::getline(in, line)) seqs.push_back(line);
  if (seqs.size() < 2) return 2;
  const EdlibAlignConfig path_cfg = edlibNewAlignConfig(-1, EDLIB_MODE_NW, EDLIB_TASK_PATH, nullptr, 0);
  {
    EdlibAlignResult r = edlibAlign("ACGT", 4, "ACGT", 4, edlibNewAlignConfig(-1, EDLIB_MODE_HW, EDLIB_TASK_PATH, nullptr, 0));
    std::printf("hw_mode_status %d\n", r.status);
    edlibFreeAlignResult(r);
  }
  {  // one known pair: cigar in both formats
    const std::string q = "ACGTTTACGGAC", t = "ACGTACGCACGG";  // 3=2I4=1X2=2D under the stated rule, distance 5
    EdlibAlignResult r = edlibAlign(q.c_str(), static_cast<int>(q.size()), t.c_str(), static_cast<int>(t.size()), path_cfg);
    if (r.status != EDLIB_STATUS_OK) {
      std::printf("NO_DEVICE status %d\n", r.status);
      return 1;
    }
    char* ext = edlibAlignmentToCigar(r.alignment, r.alignmentLength, EDLIB_CIGAR_EXTENDED);
    char* stdc = edlibAlignmentToCigar(r.alignment, r.alignmentLength, EDLIB_CIGAR_STANDARD);
    std::printf("known check %d distance %d cigar %s %s\n", check_path(r, q, t), r.editDistance, ext ? ext : "(null)", stdc ? stdc : "(null)");
    std::free(ext);
    std::free(stdc);
    edlibFreeAlignResult(r);
  }
  // pairs (i, i + 1) from 8 threads: PATH for two of three, DISTANCE for the third
  const size_t n_pairs = seqs.size() - 1;
  std::vector<int> verdict(n_pairs, -1);
  std::vector<std::thread> pool;
  for (unsigned th = 0; th < 8; ++th)
    pool.emplace_back([&, th]() {
      for (size_t i = th; i < n_pairs; i += 8) {
        const std::string &q = seqs[i], &t = seqs[i + 1];
        if (i % 3 == 2) {
          EdlibAlignResult r = edlibAlign(q.c_str(), static_cast<int>(q.size()), t.c_str(), static_cast<int>(t.size()), edlibDefaultAlignConfig());
          std::vector<unsigned char> ops;
          verdict[i] = (r.status == EDLIB_STATUS_OK && r.editDistance == dp_path(q, t, &ops) && !r.alignment && !r.startLocations) ? 0 : 20;
          edlibFreeAlignResult(r);
        } else {
          EdlibAlignResult r = edlibAlign(q.c_str(), static_cast<int>(q.size()), t.c_str(), static_cast<int>(t.size()), path_cfg);
          verdict[i] = check_path(r, q, t);
          edlibFreeAlignResult(r);
        }
      }
    });
  for (auto& th : pool) th.join();
  size_t bad = 0;
  int first_bad = 0;
  for (size_t i = 0; i < n_pairs; ++i)
    if (verdict[i] != 0) {
      if (!bad) first_bad = verdict[i];
      ++bad;
    }
  std::printf("pairs %zu bad %zu first_bad %d\n", n_pairs, bad, first_bad);
  {  // k below and at the distance; the LOC task
    const std::string &q = seqs[0], &t = seqs[1];
    std::vector<unsigned char> ops;
    const int d = dp_path(q, t, &ops);
    EdlibAlignResult r = edlibAlign(q.c_str(), static_cast<int>(q.size()), t.c_str(), static_cast<int>(t.size()),
                                    edlibNewAlignConfig(std::max(0, d - 1), EDLIB_MODE_NW, EDLIB_TASK_PATH, nullptr, 0));
    std::printf("k_below %d %d %d\n", d > 0 ? r.editDistance : -1, r.alignment == nullptr, r.numLocations);
    edlibFreeAlignResult(r);
    r = edlibAlign(q.c_str(), static_cast<int>(q.size()), t.c_str(), static_cast<int>(t.size()),
                   edlibNewAlignConfig(d, EDLIB_MODE_NW, EDLIB_TASK_PATH, nullptr, 0));
    std::printf("k_equal %d\n", check_path(r, q, t));
    edlibFreeAlignResult(r);
    r = edlibAlign(q.c_str(), static_cast<int>(q.size()), t.c_str(), static_cast<int>(t.size()),
                   edlibNewAlignConfig(-1, EDLIB_MODE_NW, EDLIB_TASK_LOC, nullptr, 0));
    std::printf("loc %d %d %d %d %d\n", r.status, r.editDistance == d, r.numLocations, r.startLocations ? r.startLocations[0] : -1,
                r.endLocations ? r.endLocations[0] == static_cast<int>(t.size()) - 1 : -1);
    std::printf("loc_no_alignment %d\n", r.alignment == nullptr && r.alignmentLength == 0);
    edlibFreeAlignResult(r);
  }
  return 0;
}
