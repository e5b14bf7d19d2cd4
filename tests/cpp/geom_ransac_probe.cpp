// Host probe of the RANSAC scan in mrs_optic_flow_amd/csrc/geom_core.hpp: replays find_homography_host's loop (mof_geom.hip) through
// ransac_hypothesis / ransac_accept and reports where it ended, so that tests can PROVE which device paths a scene reaches (a best
// model from a later round of 64, a cut between rounds). Host only, built with -ffp-contract=off like the library's geometry file.
// out: best_iter (-1: none, or n <= 4: no scan), final niters, how often the best model changed, in how many different rounds.
#include "../../mrs_optic_flow_amd/csrc/geom_core.hpp"

using namespace mof::geom;

extern "C" void geom_ransac_probe(const double* a, const double* b, int n, int* out) {
  const double thr2 = kRansacThreshold * kRansacThreshold;
  RansacScan scan{0, -1, kRansacMaxIters};
  int changes = 0, rounds = 0, last_round = -1;
  bool running = n > 4;
  for (int iter = 0; iter < kRansacMaxIters && running && iter < scan.niters; ++iter) {
    double Hk[9];
    const int cnt = ransac_hypothesis(a, b, n, kRansacSeed, iter, thr2, Hk);
    const int before = scan.best_iter;
    running = ransac_accept(&scan, iter, cnt, n);
    if (scan.best_iter == before) continue;
    ++changes;
    if (iter / kRansacBatch != last_round) ++rounds, last_round = iter / kRansacBatch;
  }
  out[0] = scan.best_iter, out[1] = scan.niters, out[2] = changes, out[3] = rounds;
}
