// mcpar-run -- the BASELINE configurations as a first-class driver (the reference reaches them
// only through its library API: SURVEY fact 3).
//   mcpar-run [--func rosen1|rosen2|rosen2fixed|gauss|dgauss|mix | --func-source FILE.hip [--par a,b,...]] [--np D]
//             [--nc CHAINS] [--nsamp N] [--nburn B] [--pl P] [--sync S] [--ncomp K] [--quiet] [--iter] [--binary]
//             [--stream-text] [--out FILE] [--summary FILE] [--rank-summary FILE] [--covariance FILE] [--proposal FILE]
//             [--incov FILE]
//             [--derive-source FILE.hip --derive-nout K [--derive-par a,b,...] | --derive-linear FILE]
//             [--derived-summary FILE] [--derived-rank-summary FILE] [--derived-covariance FILE]
//             [--draws FILE --ndraw N [--draw-seed S]]
//             [--density FILE] [--derived-density FILE] [--density-n N] [--density-clip QLO,QHI]
//             [--density2d FILE] [--derived-density2d FILE] [--density2d-n G] [--density2d-pairs a:b,c:d,...]
//             [--profile FILE] [--profile-intervals FILE] [--profile-path C,FILE] [--profile-n N] [--profile-levels p1,p2,...]
//             [--profile-clip QLO,QHI] [--profile2d FILE] [--profile2d-n G] [--profile2d-pairs a:b,c:d,...]
//             [--clip QLO,QHI] [--clip-ll-hi V] [--clip-report FILE] [--clipped FILE] [--clipped-density FILE [--clip-nc NC]]
//             [--chain-table FILE] [--chain-keep Z[,MINMOVES[,MAXSTAY]]] [--kept-chains FILE] [--kept-summary FILE]
//             [--step-table FILE [--step-probs p1,p2,...] [--settle TOLM[,TOLS[,REF]]]]
//             [--compare FILE --compare-to OTHER [--compare-nc NC]] [--compare-halves FILE] [--compare-iid]
//             [--energy FILE --compare-to OTHER [--compare-nc NC]] [--energy-halves FILE] [--energy-n NA[,NB]] [--energy-perm P]
//             [--energy-seed S] [--energy-with-ll] [--energy-raw]
//             [--mutual-info FILE] [--mi-n N] [--mi-k K] [--mi-perm P] [--mi-seed S] [--mi-pairs a:b,c:d,...] [--mi-with-ll] [--mi-raw]
//             [--reweight-temper BETA | --reweight-source FILE.hip | --reweight-logw FILE] [--reweight FILE]
//             [--resampled FILE] [--resampled-density FILE] [--resample-n K] [--resample-seed S]
//             [--intervals FILE [--hdi P1,P2,...] [--interval-probs p1,p2,...]]
//             [--mess FILE [--mess-max-lag L] [--mess-with-ll]] [--ccf FILE --ccf-lags L]
//             [--modes FILE --modes-k K [--modes-seed S] [--modes-iter M] [--modes-raw] [--modes-centres FILE]]
//             [--evidence FILE [--evidence-draws N] [--evidence-seed S] [--evidence-fit-steps F] [--evidence-modes K] [--evidence-scale S]]
//             [--mode-weights FILE] [--mode-chains FILE] [--mode-occupancy FILE] [--mode-rows K,FILE] [--mode-summary K,FILE]
//   mcpar-run --read FILE --nc NC [--np NP] [--read-skip K] [--read-rows N] [--quiet] [the analysis files above]
// --func-source: the user's own likelihood as HIP source of device functions (SourceVLFunc, MCX_VL_SOURCE: compiled into
// the engine's fused step kernels at run time; mcpar_amd/examples/ has three), --par its parameter block.
// Output: the reference's row format (src/mcout.cc:41-45); --iter prepends the iteration index
// that src/anly/mcpar-analysis.R:80-120 reconstructs; --quiet prints only the summary (stderr); --out FILE: the sample
// text goes to FILE, every rank writing its own share at its place (MCout::text_file) instead of through rank 0.
// --summary FILE: one row per column (p0 .. p{np-1}, then LL) of the kept rows' summary on the GPU (mcx_rows_summary):
// name mean sd q01 q50 q99 rhat ess mcse.  Needs the rows on the host: not with --stream-text, and one rank only.
// --rank-summary FILE: the rank-normalised diagnostics of the same rows (mcx_rows_rank_summary), one row per column: name
// rhat rhat_bulk rhat_folded ess_bulk ess_tail ess_q05 ess_q95 q05 q50 q95 ess_bulk_lag flags.  Under the conditions of
// --summary.
// --covariance FILE: mean and covariance matrix of the kept rows on the GPU (mcx_rows_covariance): header `name mean p0 ..
// LL`, then one row per column: name, mean, the matrix row.  --proposal FILE: np rows of np numbers, that matrix's
// parameter block as the proposal covariance of a next run (mcx_proposal_from_cov, scale 2.38^2 / np).  Both under the
// conditions of --summary.  --incov FILE: np * np whitespace-separated numbers, the proposal covariance of this run
// (MCPar::run's incov) -- `--proposal P.txt` of a pilot run, then `--incov P.txt`, is the adaptive two-stage job.
// --derive-source / --derive-linear: a function of one kept row (its np parameters and log L) to K derived columns
// (mcx_rows_derive; mcpar_amd/examples/derive_*.hip): a user's HIP text defining mcx_user_derive with --derive-nout outputs
// and --derive-par as its `par`, or FILE holding K rows of np + 1 numbers, a row of A and then b, for out = b + A x.
// --derived-summary, --derived-rank-summary, --derived-covariance FILE: the files of --summary, --rank-summary and
// --covariance for the derived columns d0 .. d{K-1}, then LL (mcx_store_summary, ...).  Under the conditions of --summary.
// --draws FILE --ndraw N [--draw-seed S]: N of the kept rows drawn with replacement, as the text of the sample output; the
// row of draw i is mcx_samples_draw's (mcx_debug_draw_indices of seed S, default 8675309).  Under the conditions of --summary.
// --density FILE: the kernel density estimate of every column of the kept rows on the GPU (mcx_rows_density; R's density() /
// geom_density, the reference's mcparam.density) in long form: a header `column x density`, then --density-n (default 512)
// lines `name x y` per column p0 .. LL.  --density-clip QLO,QHI: from the QLO to the QHI quantile of a column instead of min to
// max (log L keeps its maximum).  --derived-density FILE: the same for the derived columns d0 .. LL.  Both under the
// conditions of --summary.
// --density2d FILE: the joint kernel density estimate of pairs of columns of the kept rows on the GPU (mcx_rows_density2d;
// MASS::kde2d / geom_density_2d, the corner plot) in long form: a header `a b x y density`, then G * G lines `name_a name_b x y
// z` per pair, x varying slowest, with the names of --density's file.  --density2d-n G (default 64, 8 to 64): nodes per axis.
// --density2d-pairs a:b,c:d,...: these pairs of column indices (log L is np) instead of every a < b.  --density-clip applies.
// --derived-density2d FILE: the same for the derived columns d0 .. LL.  Both under the conditions of --summary.
// --clip QLO,QHI (default 0.01,0.99) and --clip-ll-hi V (default 0): the reference's mcparam.clip.tails on the GPU
// (mcx_rows_clip): the kept rows lie strictly between the QLO and QHI quantiles of every column, log L below V.
// --clip-report FILE: a header `column lo hi nbelow nabove`, one line per column p0 .. LL, then `kept K of N`.  --clipped FILE:
// the kept rows as the text of the sample output.  --clipped-density FILE [--clip-nc NC]: the file of --density for the kept
// rows, as many whole steps of NC (default 1024) pseudo-chains as they fill (mcx_rowset_store); the report's last line
// names the rows that leaves out.  All under the conditions of --summary.
// --chain-table FILE: what every chain did, on the GPU (mcx_rows_chain_table): a header, then one line per chain: its index,
// moves, longest_stay, ll_max, ll_max_step, flags, then mean sd rho1 per column p0 .. LL.  --chain-keep Z[,MINMOVES[,MAXSTAY]]
// (default 5,1,0): the rule of mcx_chains_keep over every column.  --kept-chains FILE: a header, one line `chain reasons` per
// chain (0 = kept, else 1 non-finite | 2 stuck | 4 outlier), then `kept K of NC`.  --kept-summary FILE: the file of --summary
// for the store of the kept chains (mcx_rows_select_chains, mcx_store_summary).  All under the conditions of --summary.
// --step-table FILE: what the ensemble looked like at every kept step, on the GPU (mcx_rows_step_table), in long form: a header
// `step column mean sd min q<p>... max`, then one line per (step, column p0 .. LL); a header `step moved ll_max ll_max_chain`,
// then one line per step.  The step column is the iteration the reference's mcparam.itercount puts back on every row.
// --step-probs p1,p2,... (default 0.05,0.5,0.95; up to 8): the quantiles' probabilities.  --settle TOLM[,TOLS[,REF]] (default
// 0.1,0.1,0.5): the rule of mcx_steps_settle over every column: a line `settled at step S of T` or `not settled`, a header
// `column m_ref s_ref last_out max_dev_mean max_dev_sd` and one line per column.  Under the conditions of --summary.
// --compare FILE --compare-to OTHER: do the kept rows (A) and the sample text OTHER (B: lines of np + 1 numbers from a run of NC
// chains, default --nc; parsed on the GPU) sample the same distribution?  One row per column into FILE (mcx_rows_compare, DESIGN.md
// section 20): the exact two-sample Kolmogorov-Smirnov distance, the Wasserstein-1 distance, each side's mean, sd and ESS, the z
// of the means and the Kolmogorov probability at the effective sizes (--compare-iid: at the sample sizes).  --compare-halves
// FILE: the same for the first floor(nsamp / 2) kept steps against the rest.
// --energy FILE --compare-to OTHER: the same two sides compared as clouds of points (mcx_rows_energy): the
// energy distance between NA rows of A and NB of B (--energy-n, default 0,0: min(rows, 2048) draws each; -1: every row) and its
// law under --energy-perm P (default 999) permutations of seed --energy-seed (default 0); --energy-with-ll adds log L to the
// columns, --energy-raw leaves them unscaled.  FILE: a header and one line of the result's fields, then a header `name scale
// flags` and one line per column p0 .. LL.  --energy-halves FILE: the first floor(nsamp / 2) kept steps against the rest.
// --reweight FILE: the kept rows under importance weights, on the GPU (mcx_rows_reweight).  The weight
// source is one of --reweight-temper BETA (log-weight (BETA - 1) log L: the power posterior L^BETA), --reweight-source FILE.hip
// (a derive text with one output, the log-weight of a row; --derive-par is its `par`) and --reweight-logw FILE (one number per
// row, in row order).  FILE: the first line is the global result -- n nzero lwmax sumq sumq2_hi sumq2_lo ess_kish log_mean_w
// tail_m khat tail_sigma flags --, then one line per column p0 .. LL: name mean sd mcse_mean min max q05 q50 q95 flags.
// --resampled FILE --resample-n K [--resample-seed S]: K rows drawn with replacement in proportion to the weights
// (mcx_rows_resample, seed S, default 8675309) as the text of the sample output; --resampled-density FILE: the file of
// --density for them.  All under the conditions of --summary.
// --intervals FILE: the interval estimates of the kept rows on the GPU (mcx_rows_intervals), one line per
// column p0 .. LL under a header: name mean sd mcse_sd ess_sd, then hdi<P>_lo hdi<P>_hi for every mass P of --hdi (default 0.9; up
// to 8), then q<p> mcse_q<p> ess_q<p> for every probability p of --interval-probs (default 0.05,0.5,0.95; up to 8), then flags.
// Under the conditions of --summary.
// --mess FILE: the multivariate effective sample size of the kept rows on the GPU (mcx_rows_lagcov): under a
// header one line per column p0 .. LL, name mean ess mcse flags; then one line "name value" for each of N p s k_used lags_used
// lags_computed flags mess logdet_lambda logdet_sigma; then "sigma" and the matrix, one row per line.  --mess-max-lag L: the walk
// sees lags up to L (default: all); --mess-with-ll: log L among the columns.  --ccf FILE --ccf-lags L: the cross-correlations of
// lags 0 .. L - 1, one line "lag name_i name_j ccf gamma" per (lag, i, j): column i leads column j by lag steps.  Under the
// conditions of --summary.
// --modes FILE --modes-k K: the kept rows partitioned into K modes by k-means on the GPU (mcx_rows_modes):
// one line "name value" for each of k iters flags n n_nonfinite n_changed inertia; under a header one line per mode, mode n weight
// inertia ll_mean ll_max ll_max_row flags; then "scale" and its line, then "centres", "means" and "sds" with one line per mode.
// --modes-seed S (default 0) seeds the k-means++ start, --modes-iter M bounds the passes (default 50), --modes-raw leaves the
// columns unscaled, --modes-centres FILE: K * np numbers, the centres to start from in place of the seeding.  --mode-weights FILE:
// under a header one line per mode, mode weight sd mcse_mean rhat ess (the summary of the indicator store; nsamp >= 4).
// --mode-chains FILE: under a header one line per chain, chain hops dominant dominant_steps first_label last_label and its visits
// of every mode; then "trans" and the K x K matrix.  --mode-occupancy FILE: one line per step, the step and the chains in every
// mode.  --mode-rows K,FILE: the rows of mode K as the text of the sample output.  --mode-summary K,FILE: the file of --summary for
// the rows of mode K as one sequence.  Each of them needs --modes-k (--modes FILE itself is not needed).  Under the conditions of
// --summary.
// --read FILE: no run; FILE -- sample text as --out, mcx_samples_text or the reference's drivers write it -- is parsed on
// the GPU (mcx_file_store, the reference's read.mc.data) and its rows fill the MCout the analysis files are made from: every
// one of them works on a file as on a run.  --nc NC: the chains of the run that wrote it (rows are step-major, then chain);
// --np NP: FILE has NP + 1 columns (default: those of its first line); --read-skip K: leading lines to ignore (read.table's
// skip), --read-rows N: rows to stop after (nrows).  Not with --func, --func-source, --nsamp, --nburn, --out or --stream-text.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mcpar/mcout.hh"
#include "mcpar/mcpar.hh"
#include "mcpar/rosenbrock.hh"

#include "../csrc/fmt_g6.hpp"

static const double SUMMARY_PROBS[3] = {0.01, 0.5, 0.99};

// column c of np columns and log L: p0 .. (the parameters) or d0 .. (derived columns), then LL
static std::string colname(char prefix, int c, int np) { return c < np ? prefix + std::to_string(c) : "LL"; }

// the files' writers: np named columns, then LL
static int print_summary(const char *path, const std::vector<mcx_col_summary> &cols, const std::vector<double> &q, int np, char prefix)
{
  FILE *f = fopen(path, "w");
  if (!f) {
    std::cerr << "cannot open " << path << "\n";
    return 1;
  }
  fprintf(f, "name mean sd q01 q50 q99 rhat ess mcse\n");
  for (int c = 0; c <= np; ++c) {
    const mcx_col_summary &s = cols[c];
    const double *qc = q.data() + (size_t)c * 3;
    fprintf(f, "%s %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", colname(prefix, c, np).c_str(), s.mean, s.sd, qc[0], qc[1], qc[2],
            s.rhat, s.ess, s.mcse_mean);
  }
  return fclose(f) == 0 ? 0 : 1;
}

// --summary: the per-column statistics of MCout's rows, one row per column
static int write_summary(const char *path, MCout &rows, int nsamp, int nc, int np)
{
  std::vector<mcx_col_summary> cols((size_t)np + 1);
  std::vector<double> q(((size_t)np + 1) * 3);
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 4) {
    std::cerr << "--summary: " << rows.size() << " rows stored, a summary needs nsamp * nc of them and nsamp >= 4\n";
    return 1;
  }
  if (mcx_rows_summary(rows.getpset(0), nsamp, nc, np, SUMMARY_PROBS, 3, cols.data(), q.data()) != MCX_OK) {
    std::cerr << "--summary: " << mcx_last_error() << "\n";
    return 1;
  }
  return print_summary(path, cols, q, np, 'p');
}

static int print_rank_summary(const char *path, const std::vector<mcx_col_rank_summary> &cols, int np, char prefix)
{
  FILE *f = fopen(path, "w");
  if (!f) {
    std::cerr << "cannot open " << path << "\n";
    return 1;
  }
  fprintf(f, "name rhat rhat_bulk rhat_folded ess_bulk ess_tail ess_q05 ess_q95 q05 q50 q95 ess_bulk_lag flags\n");
  for (int c = 0; c <= np; ++c) {
    const mcx_col_rank_summary &s = cols[c];
    fprintf(f, "%s %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %d\n", colname(prefix, c, np).c_str(), s.rhat, s.rhat_bulk,
            s.rhat_folded, s.ess_bulk, s.ess_tail, s.ess_q05, s.ess_q95, s.q05, s.median, s.q95, s.ess_bulk_lag, s.flags);
  }
  return fclose(f) == 0 ? 0 : 1;
}

// --rank-summary: the rank-normalised R-hat, bulk-ESS and tail-ESS of MCout's rows, one row per column
static int write_rank_summary(const char *path, MCout &rows, int nsamp, int nc, int np)
{
  std::vector<mcx_col_rank_summary> cols((size_t)np + 1);
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 4) {
    std::cerr << "--rank-summary: " << rows.size() << " rows stored, a summary needs nsamp * nc of them and nsamp >= 4\n";
    return 1;
  }
  if (mcx_rows_rank_summary(rows.getpset(0), nsamp, nc, np, cols.data()) != MCX_OK) {
    std::cerr << "--rank-summary: " << mcx_last_error() << "\n";
    return 1;
  }
  return print_rank_summary(path, cols, np, 'p');
}

// --intervals: the highest-density intervals and the Monte-Carlo errors of the sd and the quantiles of MCout's rows
static int write_intervals(const char *path, const std::vector<double> &mass, const std::vector<double> &probs, MCout &rows, int nsamp,
                           int nc, int np)
{
  const size_t ncol = (size_t)np + 1, nm = mass.size(), nq = probs.size();
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 4) {
    std::cerr << "--intervals: " << rows.size() << " rows stored, the intervals need nsamp * nc of them and nsamp >= 4\n";
    return 1;
  }
  const mcx_interval_spec spec = {(int)nm, (int)nq, mass.data(), probs.data()};
  std::vector<mcx_col_intervals> cols(ncol);
  std::vector<mcx_col_hdi> hdi(ncol * nm + 1);
  std::vector<mcx_col_quantile_se> qse(ncol * nq + 1);
  if (mcx_rows_intervals(rows.getpset(0), nsamp, nc, np, &spec, cols.data(), hdi.data(), qse.data()) != MCX_OK) {
    std::cerr << "--intervals: " << mcx_last_error() << "\n";
    return 1;
  }
  FILE *f = fopen(path, "w");
  if (!f) {
    std::cerr << "cannot open " << path << "\n";
    return 1;
  }
  fprintf(f, "name mean sd mcse_sd ess_sd");
  for (double m : mass) fprintf(f, " hdi%g_lo hdi%g_hi", m, m);
  for (double p : probs) fprintf(f, " q%g mcse_q%g ess_q%g", p, p, p);
  fprintf(f, " flags\n");
  for (size_t c = 0; c < ncol; ++c) {
    const mcx_col_intervals &s = cols[c];
    fprintf(f, "%s %.17g %.17g %.17g %.17g", colname('p', (int)c, np).c_str(), s.mean, s.sd, s.mcse_sd, s.ess_sd);
    for (size_t j = 0; j < nm; ++j) fprintf(f, " %.9g %.9g", hdi[c * nm + j].lo, hdi[c * nm + j].hi);
    for (size_t k = 0; k < nq; ++k) fprintf(f, " %.17g %.17g %.17g", qse[c * nq + k].q, qse[c * nq + k].mcse_q, qse[c * nq + k].ess_q);
    fprintf(f, " %d\n", s.flags);
  }
  return fclose(f) == 0 ? 0 : 1;
}

// --mess, --ccf: the lagged covariance of MCout's rows, the walk over it and the cross-correlations (either path may be NULL)
static int write_lagcov(const char *mess_path, const char *ccf_path, int max_lag, bool with_ll, int ccf_lags, MCout &rows, int nsamp, int nc,
                        int np)
{
  const size_t ncol = (size_t)np + 1, nn = ncol * ncol;
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 4) {
    std::cerr << "--mess / --ccf: " << rows.size() << " rows stored, the lagged covariance needs nsamp * nc of them and nsamp >= 4\n";
    return 1;
  }
  const mcx_lagcov_spec spec = {max_lag > 0 ? max_lag : nsamp - 1, ccf_path ? ccf_lags : 0, with_ll ? 1 : 0};
  mcx_lagcov_result r;
  std::vector<mcx_col_lagcov> cols(ncol);
  std::vector<double> sigma(nn), gamma(nn * (size_t)(spec.nlags_out > 0 ? spec.nlags_out : 0) + 1);
  if (mcx_rows_lagcov(rows.getpset(0), nsamp, nc, np, &spec, &r, cols.data(), sigma.data(), gamma.data()) != MCX_OK) {
    std::cerr << "--mess / --ccf: " << mcx_last_error() << "\n";
    return 1;
  }
  if (mess_path) {
    FILE *f = fopen(mess_path, "w");
    if (!f) {
      std::cerr << "cannot open " << mess_path << "\n";
      return 1;
    }
    fprintf(f, "name mean ess mcse flags\n");
    for (size_t c = 0; c < ncol; ++c)
      fprintf(f, "%s %.17g %.17g %.17g %d\n", colname('p', (int)c, np).c_str(), cols[c].mean, cols[c].ess, cols[c].mcse, cols[c].flags);
    fprintf(f, "N %lld\np %d\ns %d\nk_used %d\nlags_used %d\nlags_computed %d\nflags %d\n", r.N, r.p, r.s, r.k_used, r.lags_used,
            r.lags_computed, r.flags);
    fprintf(f, "mess %.17g\nlogdet_lambda %.17g\nlogdet_sigma %.17g\nsigma\n", r.mess, r.logdet_lambda, r.logdet_sigma);
    for (size_t i = 0; i < ncol; ++i)
      for (size_t j = 0; j < ncol; ++j) fprintf(f, "%.17g%c", sigma[i * ncol + j], j + 1 < ncol ? ' ' : '\n');
    if (fclose(f) != 0) return 1;
  }
  if (ccf_path) {
    FILE *f = fopen(ccf_path, "w");
    if (!f) {
      std::cerr << "cannot open " << ccf_path << "\n";
      return 1;
    }
    fprintf(f, "lag i j ccf gamma\n");
    for (int t = 0; t < spec.nlags_out; ++t)
      for (size_t i = 0; i < ncol; ++i)
        for (size_t j = 0; j < ncol; ++j) {
          const double vi = gamma[i * ncol + i], vj = gamma[j * ncol + j], g = gamma[(size_t)t * nn + i * ncol + j];
          const double c = !(vi > 0.0) || !(vj > 0.0) ? NAN : t == 0 && i == j ? 1.0 : g / (std::sqrt(vi) * std::sqrt(vj));
          fprintf(f, "%d %s %s %.17g %.17g\n", t, colname('p', (int)i, np).c_str(), colname('p', (int)j, np).c_str(), c, g);
        }
    if (fclose(f) != 0) return 1;
  }
  return 0;
}

static int print_covariance(const char *path, const std::vector<double> &mean, const std::vector<double> &cov, int np, char prefix)
{
  const size_t ncol = (size_t)np + 1;
  FILE *f = fopen(path, "w");
  if (!f) {
    std::cerr << "cannot open " << path << "\n";
    return 1;
  }
  fprintf(f, "name mean");
  for (int c = 0; c <= np; ++c) fprintf(f, " %s", colname(prefix, c, np).c_str());
  fprintf(f, "\n");
  for (int c = 0; c <= np; ++c) {
    fprintf(f, "%s %.17g", colname(prefix, c, np).c_str(), mean[c]);
    for (int k = 0; k <= np; ++k) fprintf(f, " %.17g", cov[c * ncol + k]);
    fprintf(f, "\n");
  }
  return fclose(f) == 0 ? 0 : 1;
}

// --covariance / --proposal: the covariance of MCout's rows, and the proposal covariance made of it
static int write_covariance(const char *cov_path, const char *prop_path, MCout &rows, int nsamp, int nc, int np)
{
  const size_t ncol = (size_t)np + 1;
  std::vector<double> mean(ncol), cov(ncol * ncol);
  if ((long long)rows.size() != (long long)nsamp * nc || (long long)nsamp * nc < 2) {
    std::cerr << "--covariance / --proposal: " << rows.size() << " rows stored, a covariance needs nsamp * nc >= 2 of them\n";
    return 1;
  }
  if (mcx_rows_covariance(rows.getpset(0), nsamp, nc, np, mean.data(), cov.data(), 0) != MCX_OK) {
    std::cerr << "--covariance / --proposal: " << mcx_last_error() << "\n";
    return 1;
  }
  if (cov_path && print_covariance(cov_path, mean, cov, np, 'p') != 0) return 1;
  if (prop_path) {
    std::vector<float> prop((size_t)np * np);
    if (mcx_proposal_from_cov(np, cov.data(), np + 1, 0.0, prop.data()) != MCX_OK) {
      std::cerr << "--proposal: " << mcx_last_error() << "\n";
      return 1;
    }
    FILE *f = fopen(prop_path, "w");
    if (!f) {
      std::cerr << "cannot open " << prop_path << "\n";
      return 1;
    }
    for (int i = 0; i < np; ++i)
      for (int j = 0; j < np; ++j) fprintf(f, "%.9g%c", prop[(size_t)i * np + j], j + 1 < np ? ' ' : '\n');
    if (fclose(f) != 0) return 1;
  }
  return 0;
}

static int print_density(const char *path, const std::vector<double> &x, const std::vector<double> &y, int np, int n, char prefix)
{
  FILE *f = fopen(path, "w");
  if (!f) {
    std::cerr << "cannot open " << path << "\n";
    return 1;
  }
  fprintf(f, "column x density\n");
  for (int c = 0; c <= np; ++c)
    for (int j = 0; j < n; ++j) fprintf(f, "%s %.17g %.17g\n", colname(prefix, c, np).c_str(), x[(size_t)c * n + j], y[(size_t)c * n + j]);
  return fclose(f) == 0 ? 0 : 1;
}

// --density: the density estimate of every column of MCout's rows, n lines per column
static int write_density(const char *path, const mcx_density_spec &spec, MCout &rows, int nsamp, int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || (long long)nsamp * nc < 2) {
    std::cerr << "--density: " << rows.size() << " rows stored, a density needs nsamp * nc >= 2 of them\n";
    return 1;
  }
  const size_t ncol = (size_t)np + 1, n = (size_t)(spec.n > 0 ? spec.n : 1);
  std::vector<mcx_col_density> cols(ncol);
  std::vector<double> x(ncol * n), y(ncol * n);
  if (mcx_rows_density(rows.getpset(0), nsamp, nc, np, &spec, cols.data(), x.data(), y.data()) != MCX_OK) {
    std::cerr << "--density: " << mcx_last_error() << "\n";
    return 1;
  }
  return print_density(path, x, y, np, spec.n, 'p');
}

// the long form of a pair density call: G * G lines per pair
static int print_density2d(const char *path, const std::vector<mcx_pair_density> &pairs, const std::vector<double> &axes,
                           const std::vector<double> &z, int np, int g, char prefix)
{
  FILE *f = fopen(path, "w");
  if (!f) {
    std::cerr << "cannot open " << path << "\n";
    return 1;
  }
  fprintf(f, "a b x y density\n");
  for (size_t p = 0; p < pairs.size(); ++p) {
    const std::string na = colname(prefix, pairs[p].a, np), nb = colname(prefix, pairs[p].b, np);
    const double *xa = axes.data() + (size_t)pairs[p].a * g, *xb = axes.data() + (size_t)pairs[p].b * g;
    for (int j = 0; j < g; ++j)
      for (int k = 0; k < g; ++k)
        fprintf(f, "%s %s %.17g %.17g %.17g\n", na.c_str(), nb.c_str(), xa[j], xb[k], z[(p * g + j) * g + k]);
  }
  return fclose(f) == 0 ? 0 : 1;
}

// the outputs of a pair density call of ncol columns, sized for the spec (a refused spec still gets buffers)
struct Density2dOut {
  std::vector<mcx_col_density> cols;
  std::vector<mcx_pair_density> pairs;
  std::vector<double> axes, z;
  Density2dOut(const mcx_density2d_spec &spec, size_t ncol)
  {
    const size_t g = (size_t)(spec.g > 0 && spec.g <= 64 ? spec.g : 64);
    size_t n = spec.pairs ? (size_t)(spec.npairs > 0 ? spec.npairs : 1) : ncol * (ncol - 1) / 2;
    if (n < 1 || n > 1024) n = 1;
    cols.resize(ncol);
    pairs.resize(n);
    axes.resize(ncol * g);
    z.resize(n * g * g);
  }
};

// --density2d: the joint density estimate of pairs of columns of MCout's rows
static int write_density2d(const char *path, const mcx_density2d_spec &spec, MCout &rows, int nsamp, int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || (long long)nsamp * nc < 2) {
    std::cerr << "--density2d: " << rows.size() << " rows stored, a density needs nsamp * nc >= 2 of them\n";
    return 1;
  }
  Density2dOut o(spec, (size_t)np + 1);
  if (mcx_rows_density2d(rows.getpset(0), nsamp, nc, np, &spec, o.cols.data(), o.axes.data(), o.pairs.data(), o.z.data()) != MCX_OK) {
    std::cerr << "--density2d: " << mcx_last_error() << "\n";
    return 1;
  }
  return print_density2d(path, o.pairs, o.axes, o.z, np, spec.g, 'p');
}

// --profile / --profile-intervals / --profile-path: the profile likelihood of every parameter of MCout's rows (mcx_rows_profile).
// --profile: a header `column bin cnt row xat lmax pl plh`, then a line per (column, bin); --profile-intervals: `column p drop lo hi
// lo_hull hi_hull nseg flags`, a line per (column, level); --profile-path C,FILE: `bin` and the names of the columns, then the whole
// row of every non-empty bin of column C
struct ProfileFiles {
  std::string curves, intervals, path, pairs;
  int path_col = -1;
  std::vector<double> levels;
  std::vector<int> pair_list;
  mcx_profile_spec spec = {64, 0.0, 1.0, 0, 0, 0, 0, 0};
  mcx_profile2d_spec spec2 = {32, 0.0, 1.0, 0, 0, 0, 0, 0, 0, 0};
  bool any1() const { return !curves.empty() || !intervals.empty() || !path.empty(); }
  bool any() const { return any1() || !pairs.empty(); }
};

static int write_profile(const ProfileFiles &pf, MCout &rows, int nsamp, int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || (long long)nsamp * nc < 2) {
    std::cerr << "--profile: " << rows.size() << " rows stored, a profile needs nsamp * nc >= 2 of them\n";
    return 1;
  }
  if (!pf.path.empty() && (pf.path_col < 0 || pf.path_col >= np)) {
    std::cerr << "--profile-path C,FILE: C is a parameter, 0 to " << np - 1 << "\n";
    return 1;
  }
  const size_t n = (size_t)(pf.spec.n > 0 && pf.spec.n <= 512 ? pf.spec.n : 512), ns = (size_t)np * n, ncol = (size_t)np + 1;
  const int nl = pf.spec.nlevels > 0 ? (pf.spec.nlevels <= MCX_PROFILE_MAX_LEVELS ? pf.spec.nlevels : MCX_PROFILE_MAX_LEVELS) : 2;
  std::vector<mcx_col_profile> cols(np);
  std::vector<unsigned long long> cnt(ns);
  std::vector<float> lmax(ns), xat(ns), path(pf.path.empty() ? 0 : ns * ncol);
  std::vector<long long> row(ns);
  std::vector<double> pl(ns), plh(ns);
  std::vector<mcx_profile_interval_t> iv((size_t)np * nl);
  if (mcx_rows_profile(rows.getpset(0), nsamp, nc, np, &pf.spec, cols.data(), cnt.data(), lmax.data(), row.data(), xat.data(), pl.data(),
                       plh.data(), iv.data(), path.empty() ? 0 : path.data()) != MCX_OK) {
    std::cerr << "--profile: " << mcx_last_error() << "\n";
    return 1;
  }
  if (!pf.curves.empty()) {
    FILE *f = fopen(pf.curves.c_str(), "w");
    if (!f) {
      std::cerr << "cannot open " << pf.curves << "\n";
      return 1;
    }
    fprintf(f, "column bin cnt row xat lmax pl plh\n");
    for (int c = 0; c < np; ++c)
      for (size_t j = 0; j < n; ++j) {
        const size_t i = (size_t)c * n + j;
        fprintf(f, "%s %zu %llu %lld %.9g %.9g %.17g %.17g\n", colname('p', c, np).c_str(), j, cnt[i], row[i], xat[i], lmax[i], pl[i], plh[i]);
      }
    if (fclose(f) != 0) return 1;
  }
  if (!pf.intervals.empty()) {
    FILE *f = fopen(pf.intervals.c_str(), "w");
    if (!f) {
      std::cerr << "cannot open " << pf.intervals << "\n";
      return 1;
    }
    fprintf(f, "column p drop lo hi lo_hull hi_hull nseg flags\n");
    for (int c = 0; c < np; ++c)
      for (int l = 0; l < nl; ++l) {
        const mcx_profile_interval_t &v = iv[(size_t)c * nl + l];
        fprintf(f, "%s %.17g %.17g %.17g %.17g %.17g %.17g %d %d\n", colname('p', c, np).c_str(), v.p, v.drop, v.lo, v.hi, v.lo_hull,
                v.hi_hull, v.nseg, v.flags);
      }
    if (fclose(f) != 0) return 1;
  }
  if (!pf.path.empty()) {
    FILE *f = fopen(pf.path.c_str(), "w");
    if (!f) {
      std::cerr << "cannot open " << pf.path << "\n";
      return 1;
    }
    fprintf(f, "bin");
    for (int c = 0; c <= np; ++c) fprintf(f, " %s", colname('p', c, np).c_str());
    fprintf(f, "\n");
    for (size_t j = 0; j < n; ++j) {
      const size_t i = (size_t)pf.path_col * n + j;
      if (row[i] < 0) continue;
      fprintf(f, "%zu", j);
      for (size_t c = 0; c < ncol; ++c) fprintf(f, " %.9g", path[i * ncol + c]);
      fprintf(f, "\n");
    }
    if (fclose(f) != 0) return 1;
  }
  return 0;
}

// --profile2d: the profile likelihood over the cells of pairs of parameters (mcx_rows_profile2d): a header `a b ia ib cnt row xat_a
// xat_b lmax z`, then a line per (pair, cell), ia varying slowest
static int write_profile2d(const ProfileFiles &pf, MCout &rows, int nsamp, int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || (long long)nsamp * nc < 2) {
    std::cerr << "--profile2d: " << rows.size() << " rows stored, a profile needs nsamp * nc >= 2 of them\n";
    return 1;
  }
  const mcx_profile2d_spec &sp = pf.spec2;
  const size_t g = (size_t)(sp.g > 0 && sp.g <= 64 ? sp.g : 64);
  size_t npairs = sp.pairs ? (size_t)(sp.npairs > 0 ? sp.npairs : 1) : (size_t)np * (np - 1) / 2;
  if (npairs < 1 || npairs > 1024) npairs = 1;
  const size_t ns = npairs * g * g;
  std::vector<mcx_col_profile> cols(np);
  std::vector<mcx_pair_profile> po(npairs);
  std::vector<unsigned long long> cnt(ns);
  std::vector<float> lmax(ns), xa(ns), xb(ns);
  std::vector<long long> row(ns), nlev(npairs * MCX_PROFILE_MAX_LEVELS);
  std::vector<double> z(ns);
  if (mcx_rows_profile2d(rows.getpset(0), nsamp, nc, np, &sp, cols.data(), po.data(), cnt.data(), lmax.data(), row.data(), xa.data(), xb.data(),
                         z.data(), nlev.data()) != MCX_OK) {
    std::cerr << "--profile2d: " << mcx_last_error() << "\n";
    return 1;
  }
  FILE *f = fopen(pf.pairs.c_str(), "w");
  if (!f) {
    std::cerr << "cannot open " << pf.pairs << "\n";
    return 1;
  }
  fprintf(f, "a b ia ib cnt row xat_a xat_b lmax z\n");
  for (size_t p = 0; p < npairs; ++p) {
    const std::string na = colname('p', po[p].a, np), nb = colname('p', po[p].b, np);
    for (size_t j = 0; j < g; ++j)
      for (size_t k = 0; k < g; ++k) {
        const size_t i = (p * g + j) * g + k;
        fprintf(f, "%s %s %zu %zu %llu %lld %.9g %.9g %.9g %.17g\n", na.c_str(), nb.c_str(), j, k, cnt[i], row[i], xa[i], xb[i], lmax[i], z[i]);
      }
  }
  return fclose(f) == 0 ? 0 : 1;
}

// --clip-report / --clipped / --clipped-density: one clip of MCout's rows, the row set's files
static int write_clip(const mcx_clip_spec &spec, const char *report_path, const char *rows_path, const char *dens_path, int clip_nc,
                      const mcx_density_spec &dspec, MCout &rows, int nsamp, int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 1) {
    std::cerr << "--clip-*: " << rows.size() << " rows stored, a clip needs nsamp * nc of them\n";
    return 1;
  }
  const size_t ncol = (size_t)np + 1;
  std::vector<mcx_col_clip> cols(ncol);
  long long K = 0;
  mcx_rowset *rs = 0;
  if (mcx_rows_clip(rows.getpset(0), nsamp, nc, np, &spec, cols.data(), &K, &rs) != MCX_OK) {
    std::cerr << "--clip: " << mcx_last_error() << "\n";
    return 1;
  }
  int rc = 0;
  const long long dsteps = clip_nc > 0 ? K / clip_nc : 0, drows = dsteps * clip_nc;
  if (rows_path) {
    FILE *f = fopen(rows_path, "w");
    if (!f) {
      std::cerr << "cannot open " << rows_path << "\n";
      rc = 1;
    }
    const long long chunk = 65536;
    std::vector<float> part;
    std::vector<char> text;
    for (long long done = 0; rc == 0 && done < K; done += chunk) {
      const long long k = K - done < chunk ? K - done : chunk;
      size_t nb = 0;
      part.resize((size_t)k * ncol);
      if (mcx_rowset_copy(rs, done, k, part.data()) != MCX_OK || mcx_format_rows(part.data(), (size_t)k, (int)ncol, 0, 0, &nb) != MCX_OK) {
        std::cerr << "--clipped: " << mcx_last_error() << "\n";
        rc = 1;
        break;
      }
      text.resize(nb);
      if (mcx_format_rows(part.data(), (size_t)k, (int)ncol, text.data(), nb, &nb) != MCX_OK) {
        std::cerr << "--clipped: " << mcx_last_error() << "\n";
        rc = 1;
      } else if (fwrite(text.data(), 1, nb, f) != nb) rc = 1;
    }
    if (f && fclose(f) != 0) rc = 1;
  }
  if (rc == 0 && dens_path) {
    mcx_store *st = 0;
    if (dsteps < 1 || dsteps > 2000000000LL) {
      std::cerr << "--clipped-density: " << K << " kept rows do not fill one step of --clip-nc " << clip_nc << " pseudo-chains\n";
      rc = 1;
    } else if (mcx_rowset_store(rs, 0, (int)dsteps, clip_nc, &st) != MCX_OK) {
      std::cerr << "--clipped-density: " << mcx_last_error() << "\n";
      rc = 1;
    } else {
      const size_t n = (size_t)(dspec.n > 0 ? dspec.n : 1);
      std::vector<mcx_col_density> dc(ncol);
      std::vector<double> x(ncol * n), y(ncol * n);
      if (mcx_store_density(st, &dspec, dc.data(), x.data(), y.data()) != MCX_OK) {
        std::cerr << "--clipped-density: " << mcx_last_error() << "\n";
        rc = 1;
      } else rc = print_density(dens_path, x, y, np, dspec.n, 'p');
      mcx_store_destroy(st);
    }
  }
  if (rc == 0 && report_path) {
    FILE *f = fopen(report_path, "w");
    if (!f) {
      std::cerr << "cannot open " << report_path << "\n";
      rc = 1;
    } else {
      fprintf(f, "column lo hi nbelow nabove\n");
      for (int c = 0; c <= np; ++c)
        fprintf(f, "%s %.17g %.17g %lld %lld\n", colname('p', c, np).c_str(), cols[c].lo, cols[c].hi, cols[c].nbelow, cols[c].nabove);
      fprintf(f, "kept %lld of %lld", K, (long long)nsamp * nc);
      if (dens_path) fprintf(f, ", density of %lld rows (%lld x %d), %lld left out", drows, dsteps, clip_nc, K - drows);
      fprintf(f, "\n");
      if (fclose(f) != 0) rc = 1;
    }
  }
  mcx_rowset_destroy(rs);
  return rc;
}

// --evidence FILE: log Z of the sampled function by bridge sampling on the GPU (mcx_rows_evidence), after a
// run on its rows and its likelihood, or after --read on the file's rows and the likelihood the likelihood flags name (--func,
// --func-source, --par, --ncomp: with --evidence they do not start a run).  FILE holds the fields of mcx_evidence_result, one
// `name value` per line, doubles with 17 significant digits.  The proposal is one Gaussian fitted on the first F steps
// (--evidence-fit-steps, default nsamp / 2), which are then left out; with --evidence-modes K it is K Gaussians, the modes of those
// first F steps (section 25, seed 0) with their weights, means and section 10's covariance of each mode's rows.  --evidence-draws N
// (default min(rows, 2^20)), --evidence-seed S (default 0), --evidence-scale S (default 1) scales the proposal's standard deviations.
struct EvidenceOpts {
  std::string file;
  long long ndraw = 0;
  unsigned seed = 0;
  int fit_steps = -1, modes_k = 0;
  double scale = 1.0;
  bool any_option = false;
};

static int evidence_host_fn(void *ctx, int npset, const float *x, float *y) { return (*static_cast<VLFunc *>(ctx))(npset, x, y); }

static int write_evidence(const EvidenceOpts &eo, VLFunc *L, MCout &rows, int nsamp, int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 1) {
    std::cerr << "--evidence: " << rows.size() << " rows stored, the evidence needs nsamp * nc of them\n";
    return 1;
  }
  mcx_vlfunc f;
  if (!L->device_descriptor(np, &f)) f = mcx_vlfunc{MCX_VL_HOST, np, 0, 0, evidence_host_fn, L};
  const int fit = eo.fit_steps >= 0 ? eo.fit_steps : nsamp / 2;
  mcx_evidence_spec spec = {eo.ndraw, eo.seed, fit, 1, 1000, 1e-10, eo.scale};
  mcx_evidence_mixture mix = {eo.modes_k, 0, 0, 0, 0, eo.scale};
  std::vector<double> wts, means, covs;
  if (eo.modes_k > 0) {  // the proposal from the modes of the fitting steps
    const int K = eo.modes_k;
    if (K > MCX_EVIDENCE_MAX_K || fit < 1) {
      std::cerr << "--evidence-modes " << K << ": 1 to " << MCX_EVIDENCE_MAX_K << " modes, fitted on at least one step\n";
      return 1;
    }
    const size_t knp = (size_t)K * np, ncol = (size_t)np + 1;
    mcx_modes_spec ms = {K, 50, 1, 16384, 0u, 0};
    mcx_modes_result mr;
    std::vector<mcx_mode_row> table((size_t)K);
    std::vector<double> cs(knp), c(knp), sds(knp), scale((size_t)np), mean(ncol), cov(ncol * ncol);
    means.resize(knp);
    wts.resize((size_t)K);
    covs.resize(knp * np);
    mcx_modes *m = 0;
    if (mcx_rows_modes(rows.getpset(0), fit, nc, np, &ms, &mr, table.data(), cs.data(), c.data(), means.data(), sds.data(), scale.data(), &m) !=
        MCX_OK) {
      std::cerr << "--evidence-modes: " << mcx_last_error() << "\n";
      return 1;
    }
    int rc = 0;
    for (int k = 0; rc == 0 && k < K; ++k) {
      mcx_rowset *rs = 0;
      mcx_store *st = 0;
      long long n = 0;
      wts[k] = table[k].weight;
      if (mcx_rows_mode_rows(rows.getpset(0), fit, nc, np, m, k, &rs) != MCX_OK || mcx_rowset_shape(rs, &n, 0, 0) != MCX_OK ||
          n >= (1ll << 31) || mcx_rowset_store(rs, 0, (int)n, 1, &st) != MCX_OK || mcx_store_covariance(st, mean.data(), cov.data(), 0) != MCX_OK) {
        std::cerr << "--evidence-modes: mode " << k << ": " << mcx_last_error() << "\n";
        rc = 1;
      }
      for (int i = 0; rc == 0 && i < np; ++i)
        for (int j = 0; j < np; ++j) covs[((size_t)k * np + i) * np + j] = cov[(size_t)i * ncol + j];
      mcx_store_destroy(st);
      mcx_rowset_destroy(rs);
    }
    mcx_modes_destroy(m);
    if (rc != 0) return rc;
    mix.weights = wts.data();
    mix.centres = means.data();
    mix.covs = covs.data();
  }
  mcx_evidence_result r;
  if (mcx_rows_evidence(rows.getpset(0), nsamp, nc, np, &f, &spec, eo.modes_k > 0 ? &mix : 0, &r) != MCX_OK) {
    std::cerr << "--evidence: " << mcx_last_error() << "\n";
    return 1;
  }
  FILE *o = fopen(eo.file.c_str(), "w");
  if (!o) {
    std::cerr << "cannot open " << eo.file << "\n";
    return 1;
  }
  fprintf(o, "n1 %lld\nn2 %lld\nk %d\nfit_steps %d\nneff %.17g\nlstar %.17g\nlog_z %.17g\nse %.17g\nre2_draws %.17g\nre2_rows %.17g\n", r.n1,
          r.n2, r.k, r.fit_steps, r.neff, r.lstar, r.log_z, r.se, r.re2_draws, r.re2_rows);
  fprintf(o, "ess_f2 %.17g\nlog_z_is %.17g\nlog_z_ris %.17g\nndraw_zero %lld\niters %d\nflags %d\n", r.ess_f2, r.log_z_is, r.log_z_ris,
          r.ndraw_zero, r.iters, r.flags);
  return fclose(o) != 0 ? 1 : 0;
}

// --modes and its companions: one modes call on MCout's rows (mcx_rows_modes), the files made of its tables and labels
struct ModesFiles {
  std::string modes, weights, chains, occupancy, rows, summary, centres;  // (centres: read, not written)
  int rows_k = -1, summary_k = -1;
  bool any() const { return !modes.empty() || !weights.empty() || !chains.empty() || !occupancy.empty() || !rows.empty() || !summary.empty(); }
};

static int write_rowset_text(const char *what, const char *path, mcx_rowset *rs, long long K, size_t ncol)
{
  FILE *f = fopen(path, "w");
  if (!f) {
    std::cerr << "cannot open " << path << "\n";
    return 1;
  }
  int rc = 0;
  const long long chunk = 65536;
  std::vector<float> part;
  std::vector<char> text;
  for (long long done = 0; rc == 0 && done < K; done += chunk) {
    const long long k = K - done < chunk ? K - done : chunk;
    size_t nb = 0;
    part.resize((size_t)k * ncol);
    if (mcx_rowset_copy(rs, done, k, part.data()) != MCX_OK || mcx_format_rows(part.data(), (size_t)k, (int)ncol, 0, 0, &nb) != MCX_OK) {
      std::cerr << what << ": " << mcx_last_error() << "\n";
      rc = 1;
      break;
    }
    text.resize(nb);
    if (mcx_format_rows(part.data(), (size_t)k, (int)ncol, text.data(), nb, &nb) != MCX_OK) {
      std::cerr << what << ": " << mcx_last_error() << "\n";
      rc = 1;
    } else if (fwrite(text.data(), 1, nb, f) != nb) rc = 1;
  }
  if (fclose(f) != 0) rc = 1;
  return rc;
}

static int write_modes(const ModesFiles &mf, mcx_modes_spec spec, MCout &rows, int nsamp, int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 1) {
    std::cerr << "--modes: " << rows.size() << " rows stored, the modes need nsamp * nc of them\n";
    return 1;
  }
  const int K = spec.k;
  std::vector<double> given;
  if (!mf.centres.empty()) {
    std::ifstream in(mf.centres.c_str());
    double v;
    while (in >> v) given.push_back(v);
    if (K < 1 || given.size() != (size_t)K * np) {
      std::cerr << "--modes-centres " << mf.centres << ": " << given.size() << " numbers, --modes-k * np = " << (long long)K * np << " are needed\n";
      return 1;
    }
    spec.centres = given.data();
  }
  const size_t kk = (size_t)(K > 0 ? K : 1), knp = kk * np;
  mcx_modes_result res;
  std::vector<mcx_mode_row> table(kk);
  std::vector<double> cs(knp), c(knp), means(knp), sds(knp), scale((size_t)np);
  mcx_modes *m = 0;
  if (mcx_rows_modes(rows.getpset(0), nsamp, nc, np, &spec, &res, table.data(), cs.data(), c.data(), means.data(), sds.data(), scale.data(),
                     &m) != MCX_OK) {
    std::cerr << "--modes: " << mcx_last_error() << "\n";
    return 1;
  }
  int rc = 0;
  auto open_w = [&](const std::string &path) -> FILE * {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) {
      std::cerr << "cannot open " << path << "\n";
      rc = 1;
    }
    return f;
  };
  auto matrix = [&](FILE *f, const char *name, const std::vector<double> &v) {
    fprintf(f, "%s\n", name);
    for (int k = 0; k < K; ++k) {
      for (int j = 0; j < np; ++j) fprintf(f, "%s%.17g", j ? " " : "", v[(size_t)k * np + j]);
      fprintf(f, "\n");
    }
  };
  if (!mf.modes.empty()) {
    if (FILE *f = open_w(mf.modes)) {
      fprintf(f, "k %d\niters %d\nflags %d\nn %lld\nn_nonfinite %lld\nn_changed %lld\ninertia %.17g\n", res.k, res.iters, res.flags, res.n,
              res.n_nonfinite, res.n_changed, res.inertia);
      fprintf(f, "mode n weight inertia ll_mean ll_max ll_max_row flags\n");
      for (int k = 0; k < K; ++k)
        fprintf(f, "%d %lld %.17g %.17g %.17g %.9g %lld %d\n", k, table[k].n, table[k].weight, table[k].inertia, table[k].ll_mean,
                (double)table[k].ll_max, table[k].ll_max_row, table[k].flags);
      fprintf(f, "scale\n");
      for (int j = 0; j < np; ++j) fprintf(f, "%s%.17g", j ? " " : "", scale[j]);
      fprintf(f, "\n");
      matrix(f, "centres", c);
      matrix(f, "means", means);
      matrix(f, "sds", sds);
      if (fclose(f) != 0) rc = 1;
    }
  }
  if (rc == 0 && !mf.weights.empty()) {
    mcx_store *st = 0;
    std::vector<mcx_col_summary> sc(kk + 1);
    if (mcx_modes_indicator_store(m, &st) != MCX_OK || mcx_store_summary(st, 0, 0, sc.data(), 0) != MCX_OK) {
      std::cerr << "--mode-weights: " << mcx_last_error() << "\n";
      rc = 1;
    } else if (FILE *f = open_w(mf.weights)) {
      fprintf(f, "mode weight sd mcse_mean rhat ess\n");
      for (int k = 0; k < K; ++k)
        fprintf(f, "%d %.17g %.17g %.17g %.17g %.17g\n", k, sc[k].mean, sc[k].sd, sc[k].mcse_mean, sc[k].rhat, sc[k].ess);
      if (fclose(f) != 0) rc = 1;
    }
    mcx_store_destroy(st);
  }
  if (rc == 0 && (!mf.chains.empty() || !mf.occupancy.empty())) {
    std::vector<mcx_mode_chain> ch((size_t)nc);
    std::vector<long long> visits((size_t)nc * kk), trans(kk * kk), occ((size_t)nsamp * kk);
    if (mcx_modes_chain_table(m, ch.data(), visits.data(), trans.data(), occ.data()) != MCX_OK) {
      std::cerr << "--mode-chains: " << mcx_last_error() << "\n";
      rc = 1;
    }
    if (rc == 0 && !mf.chains.empty())
      if (FILE *f = open_w(mf.chains)) {
        fprintf(f, "chain hops dominant dominant_steps first_label last_label visits\n");
        for (int i = 0; i < nc; ++i) {
          fprintf(f, "%d %lld %d %lld %d %d", i, ch[i].hops, ch[i].dominant, ch[i].dominant_steps, ch[i].first_label, ch[i].last_label);
          for (int k = 0; k < K; ++k) fprintf(f, " %lld", visits[(size_t)i * K + k]);
          fprintf(f, "\n");
        }
        fprintf(f, "trans\n");
        for (int a = 0; a < K; ++a) {
          for (int b = 0; b < K; ++b) fprintf(f, "%s%lld", b ? " " : "", trans[(size_t)a * K + b]);
          fprintf(f, "\n");
        }
        if (fclose(f) != 0) rc = 1;
      }
    if (rc == 0 && !mf.occupancy.empty())
      if (FILE *f = open_w(mf.occupancy)) {
        for (int t = 0; t < nsamp; ++t) {
          fprintf(f, "%d", t);
          for (int k = 0; k < K; ++k) fprintf(f, " %lld", occ[(size_t)t * K + k]);
          fprintf(f, "\n");
        }
        if (fclose(f) != 0) rc = 1;
      }
  }
  if (rc == 0 && !mf.rows.empty()) {
    mcx_rowset *rs = 0;
    long long n = 0;
    if (mcx_rows_mode_rows(rows.getpset(0), nsamp, nc, np, m, mf.rows_k, &rs) != MCX_OK || mcx_rowset_shape(rs, &n, 0, 0) != MCX_OK) {
      std::cerr << "--mode-rows: " << mcx_last_error() << "\n";
      rc = 1;
    } else rc = write_rowset_text("--mode-rows", mf.rows.c_str(), rs, n, (size_t)np + 1);
    mcx_rowset_destroy(rs);
  }
  if (rc == 0 && !mf.summary.empty()) {
    // the rows of the mode as one pseudo-chain: the file of --summary for them (its R-hat and ESS are of that one sequence)
    mcx_rowset *rs = 0;
    mcx_store *st = 0;
    long long n = 0;
    std::vector<mcx_col_summary> sc((size_t)np + 1);
    std::vector<double> q(((size_t)np + 1) * 3);
    if (mcx_rows_mode_rows(rows.getpset(0), nsamp, nc, np, m, mf.summary_k, &rs) != MCX_OK || mcx_rowset_shape(rs, &n, 0, 0) != MCX_OK) {
      std::cerr << "--mode-summary: " << mcx_last_error() << "\n";
      rc = 1;
    } else if (n < 4 || n > 2000000000LL) {
      std::cerr << "--mode-summary: mode " << mf.summary_k << " has " << n << " rows, a summary needs at least 4\n";
      rc = 1;
    } else if (mcx_rowset_store(rs, 0, (int)n, 1, &st) != MCX_OK || mcx_store_summary(st, SUMMARY_PROBS, 3, sc.data(), q.data()) != MCX_OK) {
      std::cerr << "--mode-summary: " << mcx_last_error() << "\n";
      rc = 1;
    } else rc = print_summary(mf.summary.c_str(), sc, q, np, 'p');
    mcx_store_destroy(st);
    mcx_rowset_destroy(rs);
  }
  mcx_modes_destroy(m);
  return rc;
}

// --chain-table / --kept-chains / --kept-summary: the chain table of MCout's rows, the rule's verdict on every chain and the
// summary of the store of the chains it keeps
static int write_chains(const mcx_chain_rule &rule, const char *table_path, const char *kept_path, const char *sum_path, MCout &rows,
                        int nsamp, int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 1) {
    std::cerr << "--chain-*: " << rows.size() << " rows stored, a chain table needs nsamp * nc of them\n";
    return 1;
  }
  const int ncol = np + 1;
  std::vector<mcx_chain_col> cols((size_t)nc * ncol);
  std::vector<mcx_chain_row> chains((size_t)nc);
  if (mcx_rows_chain_table(rows.getpset(0), nsamp, nc, np, cols.data(), chains.data()) != MCX_OK) {
    std::cerr << "--chain-table: " << mcx_last_error() << "\n";
    return 1;
  }
  if (table_path) {
    FILE *f = fopen(table_path, "w");
    if (!f) {
      std::cerr << "cannot open " << table_path << "\n";
      return 1;
    }
    fprintf(f, "chain moves longest_stay ll_max ll_max_step flags");
    for (int c = 0; c < ncol; ++c) {
      const std::string n = colname('p', c, np);
      fprintf(f, " %s_mean %s_sd %s_rho1", n.c_str(), n.c_str(), n.c_str());
    }
    fprintf(f, "\n");
    for (int k = 0; k < nc; ++k) {
      const mcx_chain_row &r = chains[k];
      fprintf(f, "%d %lld %lld %.9g %d %d", k, r.moves, r.longest_stay, (double)r.ll_max, r.ll_max_step, r.flags);
      for (int c = 0; c < ncol; ++c) {
        const mcx_chain_col &s = cols[(size_t)k * ncol + c];
        fprintf(f, " %.17g %.17g %.17g", s.mean, s.sd, s.rho1);
      }
      fprintf(f, "\n");
    }
    if (fclose(f) != 0) return 1;
  }
  if (!kept_path && !sum_path) return 0;
  std::vector<int> reasons((size_t)nc), kept;
  int nkept = 0;
  if (mcx_chains_keep(nc, ncol, cols.data(), chains.data(), &rule, reasons.data(), 0, &nkept) != MCX_OK) {
    std::cerr << "--chain-keep: " << mcx_last_error() << "\n";
    return 1;
  }
  for (int k = 0; k < nc; ++k)
    if (reasons[k] == 0) kept.push_back(k);
  if (kept_path) {
    FILE *f = fopen(kept_path, "w");
    if (!f) {
      std::cerr << "cannot open " << kept_path << "\n";
      return 1;
    }
    fprintf(f, "chain reasons\n");
    for (int k = 0; k < nc; ++k) fprintf(f, "%d %d\n", k, reasons[k]);
    fprintf(f, "kept %d of %d\n", nkept, nc);
    if (fclose(f) != 0) return 1;
  }
  if (sum_path) {
    if (nkept < 1 || nsamp < 4) {
      std::cerr << "--kept-summary: " << nkept << " chains kept over " << nsamp << " steps, a summary needs a chain and nsamp >= 4\n";
      return 1;
    }
    mcx_store *st = 0;
    if (mcx_rows_select_chains(rows.getpset(0), nsamp, nc, np, kept.data(), nkept, &st) != MCX_OK) {
      std::cerr << "--kept-summary: " << mcx_last_error() << "\n";
      return 1;
    }
    std::vector<mcx_col_summary> sc((size_t)ncol);
    std::vector<double> q((size_t)ncol * 3);
    int rc = 0;
    if (mcx_store_summary(st, SUMMARY_PROBS, 3, sc.data(), q.data()) != MCX_OK) {
      std::cerr << "--kept-summary: " << mcx_last_error() << "\n";
      rc = 1;
    } else rc = print_summary(sum_path, sc, q, np, 'p');
    mcx_store_destroy(st);
    return rc;
  }
  return 0;
}

// --step-table [--settle]: the step table of MCout's rows and the rule's verdict on it
static int write_steps(const char *path, const std::vector<double> &probs, const mcx_step_rule *rule, MCout &rows, int nsamp, int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 1) {
    std::cerr << "--step-table: " << rows.size() << " rows stored, a step table needs nsamp * nc of them\n";
    return 1;
  }
  const int ncol = np + 1, nprobs = (int)probs.size();
  std::vector<mcx_step_col> cols((size_t)nsamp * ncol);
  std::vector<mcx_step_row> steps((size_t)nsamp);
  std::vector<double> q(cols.size() * probs.size() + 1);
  if (mcx_rows_step_table(rows.getpset(0), nsamp, nc, np, probs.data(), nprobs, cols.data(), steps.data(), q.data()) != MCX_OK) {
    std::cerr << "--step-table: " << mcx_last_error() << "\n";
    return 1;
  }
  std::vector<mcx_step_settle_col> sc((size_t)ncol);
  int settled = -1;
  if (rule && mcx_steps_settle(nsamp, ncol, cols.data(), rule, sc.data(), &settled) != MCX_OK) {
    std::cerr << "--settle: " << mcx_last_error() << "\n";
    return 1;
  }
  FILE *f = fopen(path, "w");
  if (!f) {
    std::cerr << "cannot open " << path << "\n";
    return 1;
  }
  fprintf(f, "step column mean sd min");
  for (double p : probs) fprintf(f, " q%g", p);
  fprintf(f, " max\n");
  for (int t = 0; t < nsamp; ++t)
    for (int c = 0; c < ncol; ++c) {
      const size_t i = (size_t)t * ncol + c;
      fprintf(f, "%d %s %.17g %.17g %.9g", t, colname('p', c, np).c_str(), cols[i].mean, cols[i].sd, (double)cols[i].min);
      for (int k = 0; k < nprobs; ++k) fprintf(f, " %.17g", q[i * nprobs + k]);
      fprintf(f, " %.9g\n", (double)cols[i].max);
    }
  fprintf(f, "step moved ll_max ll_max_chain\n");
  for (int t = 0; t < nsamp; ++t) fprintf(f, "%d %d %.9g %d\n", t, steps[t].moved, (double)steps[t].ll_max, steps[t].ll_max_chain);
  if (rule) {
    if (settled >= 0) fprintf(f, "settled at step %d of %d\n", settled, nsamp);
    else fprintf(f, "not settled\n");
    fprintf(f, "column m_ref s_ref last_out max_dev_mean max_dev_sd\n");
    for (int c = 0; c < ncol; ++c)
      fprintf(f, "%s %.17g %.17g %d %.17g %.17g\n", colname('p', c, np).c_str(), sc[c].m_ref, sc[c].s_ref, sc[c].last_out,
              sc[c].max_dev_mean, sc[c].max_dev_sd);
  }
  return fclose(f) == 0 ? 0 : 1;
}

// one row per column of a comparison
static int print_compare(const char *path, const std::vector<mcx_col_compare> &cols, int np)
{
  FILE *f = fopen(path, "w");
  if (!f) {
    std::cerr << "cannot open " << path << "\n";
    return 1;
  }
  fprintf(f, "name ks ks_plus_num ks_plus_x ks_minus_num ks_minus_x w1 mean_a sd_a ess_a mean_b sd_b ess_b z_mean ks_neff ks_p na nb flags\n");
  for (int c = 0; c <= np; ++c) {
    const mcx_col_compare &o = cols[c];
    fprintf(f, "%s %.17g %lld %.17g %lld %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %lld %lld %d\n",
            colname('p', c, np).c_str(), o.ks, o.ks_plus_num, o.ks_plus_x, o.ks_minus_num, o.ks_minus_x, o.w1, o.mean_a, o.sd_a, o.ess_a,
            o.mean_b, o.sd_b, o.ess_b, o.z_mean, o.ks_neff, o.ks_p, o.na, o.nb, o.flags);
  }
  return fclose(f) == 0 ? 0 : 1;
}

// --compare-to OTHER: the sample text of other_nc chains parsed on the GPU -> its rows rb of tb whole steps.  The library's
// code, or -1 when the text could not be read (said on stderr)
static int read_other(const char *other, int other_nc, int np, std::vector<float> &rb, int &tb)
{
  mcx_text_spec tspec = {np + 1, other_nc, 0, -1, 0};
  mcx_text_report trep;
  mcx_store *ts = 0;
  if (mcx_file_store(other, &tspec, &ts, &trep) != MCX_OK) {
    std::cerr << "--compare-to " << other << ": " << mcx_last_error() << "\n";
    return -1;
  }
  tb = (int)(trep.nrows / other_nc);
  rb.resize((size_t)trep.nrows * (size_t)trep.ncol);
  const int rc = mcx_store_copy(ts, 0, tb, rb.data());
  mcx_store_destroy(ts);
  return rc;
}

// --compare FILE --compare-to OTHER: MCout's rows (A) against the sample text OTHER of other_nc chains (B), parsed on the GPU;
// --compare-halves FILE: the first floor(nsamp / 2) kept steps (A) against the rest (B)
static int write_compare(const char *path, const char *other, int other_nc, bool iid, const char *halves_path, MCout &rows, int nsamp,
                         int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 1) {
    std::cerr << "--compare: " << rows.size() << " rows stored, a comparison needs nsamp * nc of them\n";
    return 1;
  }
  const mcx_compare_spec spec = {iid ? MCX_COMPARE_IID : 0};
  std::vector<mcx_col_compare> cols((size_t)np + 1);
  if (path) {
    std::vector<float> rb;
    int tb = 0;
    int rc = read_other(other, other_nc, np, rb, tb);
    if (rc < 0) return 1;
    if (rc == MCX_OK) rc = mcx_rows_compare(rows.getpset(0), nsamp, nc, rb.data(), tb, other_nc, np, &spec, cols.data());
    if (rc != MCX_OK) {
      std::cerr << "--compare: " << mcx_last_error() << "\n";
      return 1;
    }
    if (print_compare(path, cols, np) != 0) return 1;
  }
  if (halves_path) {
    const int h = nsamp / 2;
    if (h < 1) {
      std::cerr << "--compare-halves: " << nsamp << " kept steps, two halves need at least 2\n";
      return 1;
    }
    if (mcx_rows_compare(rows.getpset(0), h, nc, rows.getpset(0) + (size_t)h * nc * (np + 1), nsamp - h, nc, np, &spec, cols.data()) != MCX_OK) {
      std::cerr << "--compare-halves: " << mcx_last_error() << "\n";
      return 1;
    }
    if (print_compare(halves_path, cols, np) != 0) return 1;
  }
  return 0;
}

// the result of a joint comparison and one row per column
static int print_energy(const char *path, const mcx_energy_result &r, const std::vector<mcx_energy_col> &cols, int np)
{
  FILE *f = fopen(path, "w");
  if (!f) {
    std::cerr << "cannot open " << path << "\n";
    return 1;
  }
  fprintf(f, "e h mean_ab mean_aa mean_bb p_value nge n_a n_b nperm nused na_rows nb_rows\n");
  fprintf(f, "%.17g %.17g %.17g %.17g %.17g %.17g %lld %d %d %d %d %lld %lld\n", r.e, r.h, r.mean_ab, r.mean_aa, r.mean_bb, r.p_value, r.nge,
          r.n_a, r.n_b, r.nperm, r.nused, r.na_rows, r.nb_rows);
  fprintf(f, "name scale flags\n");
  for (int c = 0; c <= np; ++c) fprintf(f, "%s %.17g %d\n", colname('p', c, np).c_str(), cols[c].scale, cols[c].flags);
  return fclose(f) == 0 ? 0 : 1;
}

// --energy FILE --compare-to OTHER: MCout's rows (A) against the sample text OTHER of other_nc chains (B);
// --energy-halves FILE: the first floor(nsamp / 2) kept steps (A) against the rest (B)
static int write_energy(const char *path, const char *other, int other_nc, const mcx_energy_spec &spec, const char *halves_path, MCout &rows,
                        int nsamp, int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 1) {
    std::cerr << "--energy: " << rows.size() << " rows stored, a comparison needs nsamp * nc of them\n";
    return 1;
  }
  mcx_energy_result res;
  std::vector<mcx_energy_col> cols((size_t)np + 1);
  if (path) {
    std::vector<float> rb;
    int tb = 0;
    int rc = read_other(other, other_nc, np, rb, tb);
    if (rc < 0) return 1;
    if (rc == MCX_OK) rc = mcx_rows_energy(rows.getpset(0), nsamp, nc, rb.data(), tb, other_nc, np, &spec, &res, cols.data(), 0);
    if (rc != MCX_OK) {
      std::cerr << "--energy: " << mcx_last_error() << "\n";
      return 1;
    }
    if (print_energy(path, res, cols, np) != 0) return 1;
  }
  if (halves_path) {
    const int h = nsamp / 2;
    if (h < 1) {
      std::cerr << "--energy-halves: " << nsamp << " kept steps, two halves need at least 2\n";
      return 1;
    }
    if (mcx_rows_energy(rows.getpset(0), h, nc, rows.getpset(0) + (size_t)h * nc * (np + 1), nsamp - h, nc, np, &spec, &res, cols.data(), 0) !=
        MCX_OK) {
      std::cerr << "--energy-halves: " << mcx_last_error() << "\n";
      return 1;
    }
    if (print_energy(halves_path, res, cols, np) != 0) return 1;
  }
  return 0;
}

// --mutual-info FILE: which columns of MCout's rows depend on each other at all (mcx_rows_mutinfo): the
// mutual information of every pair of parameters (--mi-pairs a:b,... names the pairs; --mi-with-ll adds log L) by the k-nearest-
// neighbour estimator (--mi-k, default 3) on --mi-n rows evenly spaced in store order (default 0: min(rows, 4096); -1: every row),
// scaled by their sd (--mi-raw: unscaled), under --mi-perm P (default 0) permutations of seed --mi-seed.  FILE: a header and one
// line of the result's fields, then a header `a b mi r_info pearson perm_mean perm_sd p_value nge nzero flags` and one line per pair.
// A warning goes to stderr when more than a tenth of the rows taken repeat an earlier one, or a pair has ties
static int write_mutinfo(const char *path, const mcx_mutinfo_spec &spec, MCout &rows, int nsamp, int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 1) {
    std::cerr << "--mutual-info: " << rows.size() << " rows stored, the analysis needs nsamp * nc of them\n";
    return 1;
  }
  const int used = np + ((spec.flags & MCX_MUTINFO_WITH_LL) ? 1 : 0);
  const size_t room = spec.pairs ? (size_t)std::max(spec.npairs, 1) : (size_t)std::max(used * (used - 1) / 2, 1);
  mcx_mutinfo_result res;
  std::vector<mcx_mutinfo_pair> pairs(room);
  if (mcx_rows_mutinfo(rows.getpset(0), nsamp, nc, np, &spec, &res, 0, pairs.data(), 0) != MCX_OK) {
    std::cerr << "--mutual-info: " << mcx_last_error() << "\n";
    return 1;
  }
  FILE *f = fopen(path, "w");
  if (!f) {
    std::cerr << "cannot open " << path << "\n";
    return 1;
  }
  fprintf(f, "n_rows n_sel ndup m k npairs nperm nused\n");
  fprintf(f, "%lld %d %d %d %d %d %d %d\n", res.n_rows, res.n_sel, res.ndup, res.m, res.k, res.npairs, res.nperm, res.nused);
  fprintf(f, "a b mi r_info pearson perm_mean perm_sd p_value nge nzero flags\n");
  int ties = 0;
  for (int i = 0; i < res.npairs; ++i) {
    const mcx_mutinfo_pair &o = pairs[(size_t)i];
    fprintf(f, "%s %s %.17g %.17g %.17g %.17g %.17g %.17g %lld %lld %d\n", colname('p', o.a, np).c_str(), colname('p', o.b, np).c_str(), o.mi,
            o.r_info, o.pearson, o.perm_mean, o.perm_sd, o.p_value, o.nge, o.nzero, o.flags);
    if (o.flags & MCX_MUTINFO_PAIR_TIES) ++ties;
  }
  if (res.ndup * 10 > res.n_sel)
    std::cerr << "--mutual-info: warning: " << res.ndup << " of the " << res.n_sel
              << " rows taken repeat an earlier one and were dropped: the rows are too close in time, take fewer (--mi-n)\n";
  if (ties > 0) std::cerr << "--mutual-info: warning: " << ties << " pairs have points whose k nearest neighbours are at distance 0 (flags & 4)\n";
  return fclose(f) == 0 ? 0 : 1;
}

// --reweight-temper / --reweight-source / --reweight-logw: the weight source of --reweight, --resampled and --resampled-density
struct ReweightSource {
  bool temper = false;
  double beta = 1.0;
  std::string source_file, logw_file;
  bool given() const { return temper || !source_file.empty() || !logw_file.empty(); }
};

// --reweight FILE: the rows of MCout under importance weights -- the first line is the global result (n
// nzero lwmax sumq sumq2_hi sumq2_lo ess_kish log_mean_w tail_m khat tail_sigma flags), then one row per column (name mean sd
// mcse_mean min max, the quantiles at 0.05, 0.5 and 0.95, flags); --resampled FILE: K weighted draws as sample text;
// --resampled-density FILE: their densities
static int write_reweight(const ReweightSource &src, const std::vector<float> &par, const char *path, const char *resampled_path,
                          const char *density_path, long long K, unsigned seed, const mcx_density_spec &dspec, MCout &rows, int nsamp,
                          int nc, int np)
{
  static const double probs[3] = {0.05, 0.5, 0.95};
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 1) {
    std::cerr << "--reweight: " << rows.size() << " rows stored, importance weights need nsamp * nc of them\n";
    return 1;
  }
  const size_t N = (size_t)nsamp * nc, ncol = (size_t)np + 1;
  mcx_weights w = {MCX_WEIGHT_LL, 0, 0, 0, src.beta - 1.0};
  std::vector<float> logw;
  mcx_store *ws = 0;
  if (!src.logw_file.empty()) {
    FILE *f = fopen(src.logw_file.c_str(), "r");
    if (!f) {
      std::cerr << "--reweight-logw: cannot read " << src.logw_file << "\n";
      return 1;
    }
    double t;
    while (fscanf(f, "%lf", &t) == 1) logw.push_back((float)t);
    const bool clean = feof(f) != 0;
    fclose(f);
    if (!clean || logw.size() != N) {
      std::cerr << "--reweight-logw: " << src.logw_file << " holds " << logw.size() << " numbers" << (clean ? "" : " before something that is not one")
                << ", one per row = " << N << " are needed\n";
      return 1;
    }
    w = mcx_weights{MCX_WEIGHT_HOST, logw.data(), 0, 0, 1.0};
  } else if (!src.source_file.empty()) {
    FILE *f = fopen(src.source_file.c_str(), "rb");
    if (!f) {
      std::cerr << "--reweight-source: cannot read " << src.source_file << "\n";
      return 1;
    }
    std::string text;
    char buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, k);
    fclose(f);
    const mcx_derive spec = {MCX_DERIVE_SOURCE, 1, (int)par.size(), par.empty() ? 0 : par.data(), text.c_str()};
    if (mcx_rows_derive(rows.getpset(0), nsamp, nc, np, &spec, &ws) != MCX_OK) {
      std::cerr << "--reweight-source: " << mcx_last_error() << "\n";
      return 1;
    }
    w = mcx_weights{MCX_WEIGHT_STORE, 0, ws, 0, 1.0};
  }
  int rc = 0;
  if (path) {
    mcx_reweight_result r;
    std::vector<mcx_col_reweight> cols(ncol);
    std::vector<double> q(ncol * 3);
    if (mcx_rows_reweight(rows.getpset(0), nsamp, nc, np, &w, probs, 3, &r, cols.data(), q.data()) != MCX_OK) {
      std::cerr << "--reweight: " << mcx_last_error() << "\n";
      rc = 1;
    } else {
      FILE *f = fopen(path, "w");
      if (!f) {
        std::cerr << "cannot open " << path << "\n";
        rc = 1;
      } else {
        fprintf(f, "%lld %lld %.17g %lld %llu %llu %.17g %.17g %lld %.17g %.17g %d\n", r.n, r.nzero, r.lwmax, r.sumq, r.sumq2_hi, r.sumq2_lo,
                r.ess_kish, r.log_mean_w, r.tail_m, r.khat, r.tail_sigma, r.flags);
        for (size_t c = 0; c < ncol; ++c)
          fprintf(f, "%s %.17g %.17g %.17g %.9g %.9g %.17g %.17g %.17g %d\n", colname('p', (int)c, np).c_str(), cols[c].mean, cols[c].sd,
                  cols[c].mcse_mean, (double)cols[c].min, (double)cols[c].max, q[c * 3], q[c * 3 + 1], q[c * 3 + 2], cols[c].flags);
        if (fclose(f) != 0) rc = 1;
      }
    }
  }
  if (rc == 0 && (resampled_path || density_path)) {
    // a store of K rows: as many "chains" as the largest divisor of K up to 1024 (its rows are draws, not chains)
    int nc_out = 1;
    for (int d = 1; d <= 1024 && d <= K; ++d)
      if (K % d == 0) nc_out = d;
    mcx_store *st = 0;
    if (K < 1 || K / nc_out > 2147483647LL ||
        mcx_rows_resample(rows.getpset(0), nsamp, nc, np, &w, seed, (int)(K / nc_out), nc_out, &st, 0) != MCX_OK) {
      std::cerr << "--resampled: " << (K < 1 ? "--resample-n gives the number of draws, at least 1" : mcx_last_error()) << "\n";
      rc = 1;
    }
    if (rc == 0 && resampled_path) {
      std::vector<float> drawn((size_t)K * ncol);
      size_t nb = 0;
      std::vector<char> text;
      if (mcx_store_copy(st, 0, (int)(K / nc_out), drawn.data()) != MCX_OK || mcx_format_rows(drawn.data(), (size_t)K, (int)ncol, 0, 0, &nb) != MCX_OK) rc = 1;
      if (rc == 0) {
        text.resize(nb);
        if (mcx_format_rows(drawn.data(), (size_t)K, (int)ncol, text.data(), nb, &nb) != MCX_OK) rc = 1;
      }
      if (rc != 0) std::cerr << "--resampled: " << mcx_last_error() << "\n";
      else {
        FILE *f = fopen(resampled_path, "w");
        if (!f) {
          std::cerr << "cannot open " << resampled_path << "\n";
          rc = 1;
        } else {
          if (nb && fwrite(text.data(), 1, nb, f) != nb) rc = 1;
          if (fclose(f) != 0) rc = 1;
        }
      }
    }
    if (rc == 0 && density_path) {
      const size_t n = (size_t)(dspec.n > 0 ? dspec.n : 1);
      std::vector<mcx_col_density> cols(ncol);
      std::vector<double> x(ncol * n), y(ncol * n);
      if (mcx_store_density(st, &dspec, cols.data(), x.data(), y.data()) != MCX_OK) {
        std::cerr << "--resampled-density: " << mcx_last_error() << "\n";
        rc = 1;
      } else rc = print_density(density_path, x, y, np, dspec.n, 'p');
    }
    mcx_store_destroy(st);
  }
  mcx_store_destroy(ws);
  return rc;
}

// --derived-*: the files for the K derived columns of MCout's rows, through one derived store on the device
static int write_derived(const mcx_derive &spec, const char *sum_path, const char *rank_path, const char *cov_path, const char *dens_path,
                         const mcx_density_spec &dspec, const char *dens2d_path, const mcx_density2d_spec &d2spec, MCout &rows, int nsamp,
                         int nc, int np)
{
  if ((long long)rows.size() != (long long)nsamp * nc || nsamp < 1) {
    std::cerr << "--derived-*: " << rows.size() << " rows stored, a derive needs nsamp * nc of them\n";
    return 1;
  }
  mcx_store *st = 0;
  if (mcx_rows_derive(rows.getpset(0), nsamp, nc, np, &spec, &st) != MCX_OK) {
    std::cerr << "--derive-*: " << mcx_last_error() << "\n";
    return 1;
  }
  const int K = spec.nout;
  int rc = 0;
  if (sum_path) {
    std::vector<mcx_col_summary> cols((size_t)K + 1);
    std::vector<double> q(((size_t)K + 1) * 3);
    if (mcx_store_summary(st, SUMMARY_PROBS, 3, cols.data(), q.data()) != MCX_OK) {
      std::cerr << "--derived-summary: " << mcx_last_error() << "\n";
      rc = 1;
    } else rc = print_summary(sum_path, cols, q, K, 'd');
  }
  if (rc == 0 && rank_path) {
    std::vector<mcx_col_rank_summary> cols((size_t)K + 1);
    if (mcx_store_rank_summary(st, cols.data()) != MCX_OK) {
      std::cerr << "--derived-rank-summary: " << mcx_last_error() << "\n";
      rc = 1;
    } else rc = print_rank_summary(rank_path, cols, K, 'd');
  }
  if (rc == 0 && cov_path) {
    std::vector<double> mean((size_t)K + 1), cov(((size_t)K + 1) * ((size_t)K + 1));
    if (mcx_store_covariance(st, mean.data(), cov.data(), 0) != MCX_OK) {
      std::cerr << "--derived-covariance: " << mcx_last_error() << "\n";
      rc = 1;
    } else rc = print_covariance(cov_path, mean, cov, K, 'd');
  }
  if (rc == 0 && dens_path) {
    const size_t n = (size_t)(dspec.n > 0 ? dspec.n : 1);
    std::vector<mcx_col_density> cols((size_t)K + 1);
    std::vector<double> x(((size_t)K + 1) * n), y(((size_t)K + 1) * n);
    if (mcx_store_density(st, &dspec, cols.data(), x.data(), y.data()) != MCX_OK) {
      std::cerr << "--derived-density: " << mcx_last_error() << "\n";
      rc = 1;
    } else rc = print_density(dens_path, x, y, K, dspec.n, 'd');
  }
  if (rc == 0 && dens2d_path) {
    Density2dOut o(d2spec, (size_t)K + 1);
    if (mcx_store_density2d(st, &d2spec, o.cols.data(), o.axes.data(), o.pairs.data(), o.z.data()) != MCX_OK) {
      std::cerr << "--derived-density2d: " << mcx_last_error() << "\n";
      rc = 1;
    } else rc = print_density2d(dens2d_path, o.pairs, o.axes, o.z, K, d2spec.g, 'd');
  }
  mcx_store_destroy(st);
  return rc;
}

// --derive-linear: K rows of np + 1 numbers (a row of A, then b) -> par = A[K][np], then b[K]
static int read_linear(const char *path, int np, std::vector<float> &par, int *nout)
{
  FILE *f = fopen(path, "r");
  if (!f) {
    std::cerr << "--derive-linear: cannot read " << path << "\n";
    return 1;
  }
  std::vector<double> v;
  double t;
  while (fscanf(f, "%lf", &t) == 1) v.push_back(t);
  const bool clean = feof(f) != 0;
  fclose(f);
  const size_t w = (size_t)np + 1, K = v.size() / w;
  if (!clean || K < 1 || K > 256 || K * w != v.size()) {
    std::cerr << "--derive-linear: " << path << " holds " << v.size() << " numbers" << (clean ? "" : " before something that is not one")
              << ", 1 to 256 rows of np + 1 = " << w << " are needed\n";
    return 1;
  }
  par.resize(v.size());
  for (size_t j = 0; j < K; ++j) {
    for (int k = 0; k < np; ++k) par[j * np + k] = (float)v[j * w + k];
    par[K * np + j] = (float)v[j * w + np];
  }
  *nout = (int)K;
  return 0;
}

// --draws: ndraw of MCout's rows with replacement, the rows mcx_samples_draw picks, as the text of the sample output
static int write_draws(const char *path, MCout &rows, int np, long long ndraw, unsigned seed)
{
  const size_t ncol = (size_t)np + 1;
  if (rows.size() < 1 || ndraw < 0 || ndraw > 2000000000LL) {
    std::cerr << "--draws: " << rows.size() << " rows stored, --ndraw " << ndraw << ": at least one row and 0 to 2e9 draws\n";
    return 1;
  }
  std::vector<int64_t> index((size_t)ndraw);
  if (mcx_debug_draw_indices(seed, (uint64_t)rows.size(), 0, (int)ndraw, index.data()) != MCX_OK) {
    std::cerr << "--draws: " << mcx_last_error() << "\n";
    return 1;
  }
  std::vector<float> drawn((size_t)ndraw * ncol);
  for (size_t i = 0; i < index.size(); ++i) std::memcpy(&drawn[i * ncol], rows.getpset((int)index[i]), ncol * sizeof(float));
  size_t nb = 0;
  std::vector<char> text;
  if (ndraw > 0) {
    if (mcx_format_rows(drawn.data(), (size_t)ndraw, (int)ncol, 0, 0, &nb) != MCX_OK) {
      std::cerr << "--draws: " << mcx_last_error() << "\n";
      return 1;
    }
    text.resize(nb);
    if (mcx_format_rows(drawn.data(), (size_t)ndraw, (int)ncol, text.data(), nb, &nb) != MCX_OK) {
      std::cerr << "--draws: " << mcx_last_error() << "\n";
      return 1;
    }
  }
  FILE *f = fopen(path, "w");
  if (!f) {
    std::cerr << "cannot open " << path << "\n";
    return 1;
  }
  if (nb && fwrite(text.data(), 1, nb, f) != nb) {
    fclose(f);
    return 1;
  }
  return fclose(f) == 0 ? 0 : 1;
}

// --incov: np * np numbers -> incov, checked by the factorisation MCPar::covar_setup will use
static int read_incov(const char *path, int np, std::vector<float> &incov)
{
  FILE *f = fopen(path, "r");
  if (!f) {
    std::cerr << "--incov: cannot read " << path << "\n";
    return 1;
  }
  std::vector<double> v;
  double t;
  while (fscanf(f, "%lf", &t) == 1) v.push_back(t);
  const bool clean = feof(f) != 0;
  fclose(f);
  if (!clean || v.size() != (size_t)np * np) {
    std::cerr << "--incov: " << path << " holds " << v.size() << " numbers" << (clean ? "" : " before something that is not one")
              << ", np * np = " << (size_t)np * np << " are needed\n";
    return 1;
  }
  incov.resize(v.size());
  for (size_t i = 0; i < v.size(); ++i) v[i] = (double)(incov[i] = (float)v[i]);
  std::vector<float> sym(v.size());
  if (mcx_proposal_from_cov(np, v.data(), np, 1.0, sym.data()) != MCX_OK) {
    std::cerr << "--incov: " << mcx_last_error() << "\n";
    return 1;
  }
  return 0;
}

int main(int argc, char *argv[])
{
  std::string func = "rosen1";
  int np = 16, nc = 4096, nsamp = 100, nburn = 500, sync = 10, ncomp = 8;
  float pl = 1.0f;
  bool quiet = false, iter = false, binary = false, stream_text = false;
  std::string out_file, func_source, summary_file, rank_summary_file, covariance_file, proposal_file, incov_file;
  std::string derive_source_file, derive_linear_file, derived_summary_file, derived_rank_summary_file, derived_covariance_file, draws_file;
  std::string density_file, derived_density_file, clip_report_file, clipped_file, clipped_density_file;
  mcx_clip_spec clip_spec = {0.01, 0.99, 0.0, 0, 0};
  int clip_nc = 1024;
  std::string chain_table_file, kept_chains_file, kept_summary_file;
  mcx_chain_rule chain_rule = {5.0, 1, 0, 0};
  std::string step_table_file, intervals_file, mess_file, ccf_file;
  int mess_max_lag = 0, ccf_lags = 0;
  ModesFiles modes_files;
  EvidenceOpts evidence;
  mcx_modes_spec modes_spec = {0, 50, 1, 16384, 0u, 0};
  bool mess_with_ll = false;
  std::vector<double> hdi_mass = {0.9}, interval_probs = {0.05, 0.5, 0.95};
  std::string compare_file, compare_to_file, compare_halves_file;
  int compare_nc = 0;
  bool compare_iid = false;
  std::string energy_file, energy_halves_file;
  mcx_energy_spec energy_spec = {0, 0, 999, 0u, 0u};
  bool energy_opts = false;
  std::string mutinfo_file;
  mcx_mutinfo_spec mutinfo_spec = {0, 0, 0, 0u, 0u, 0, 0};
  std::vector<int> mutinfo_pairs;
  bool mutinfo_opts = false;
  ReweightSource reweight_source;
  std::string reweight_file, resampled_file, resampled_density_file;
  long long resample_n = 0;
  unsigned resample_seed = 8675309u;
  std::vector<double> step_probs = {0.05, 0.5, 0.95};
  mcx_step_rule step_rule = {0.1, 0.1, 0.5, 0};
  bool settle = false;
  mcx_density_spec density_spec = {512, 1.0, 0.0, 1.0, 0, 0, 0};
  std::string density2d_file, derived_density2d_file;
  ProfileFiles profile_files;
  mcx_density2d_spec density2d_spec = {64, 1.0, 0.0, 1.0, 0, 0, 0, 0, 0};
  std::vector<int> density2d_pairs;
  std::vector<float> user_par, derive_par;
  int derive_nout = 0;
  long long ndraw = 0;
  unsigned draw_seed = 8675309u;
  std::string read_file, run_only, func_flag;  // run_only: the first option given that only a run takes
  bool np_given = false, nc_given = false;
  long long read_skip = 0, read_rows = -1;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto val = [&]() -> const char * { return i + 1 < argc ? argv[++i] : "0"; };
    if (run_only.empty() && (a == "--nsamp" || a == "--nburn" || a == "--out" || a == "--stream-text")) run_only = a;
    if (func_flag.empty() && (a == "--func" || a == "--func-source")) func_flag = a;  // (run-only unless --evidence wants a likelihood)
    if (a == "--func") func = val();
    else if (a == "--func-source") func_source = val();
    else if (a == "--par") {
      std::stringstream ss(val());
      for (std::string tok; std::getline(ss, tok, ',');) user_par.push_back((float)atof(tok.c_str()));
    }
    else if (a == "--np") { np = atoi(val()); np_given = true; }
    else if (a == "--nc") { nc = atoi(val()); nc_given = true; }
    else if (a == "--read") read_file = val();
    else if (a == "--read-skip") read_skip = atoll(val());
    else if (a == "--read-rows") read_rows = atoll(val());
    else if (a == "--nsamp") nsamp = atoi(val());
    else if (a == "--nburn") nburn = atoi(val());
    else if (a == "--pl") pl = (float)atof(val());
    else if (a == "--sync") sync = atoi(val());
    else if (a == "--ncomp") ncomp = atoi(val());
    else if (a == "--quiet") quiet = true;
    else if (a == "--iter") iter = true;
    else if (a == "--binary") binary = true;  // rows as raw float32 (np+1 per row) instead of text
    else if (a == "--stream-text") stream_text = true;  // the same text, formatted on the GPU, nothing kept on the host
    else if (a == "--out") out_file = val();
    else if (a == "--summary") summary_file = val();
    else if (a == "--rank-summary") rank_summary_file = val();
    else if (a == "--covariance") covariance_file = val();
    else if (a == "--proposal") proposal_file = val();
    else if (a == "--incov") incov_file = val();
    else if (a == "--derive-source") derive_source_file = val();
    else if (a == "--derive-nout") derive_nout = atoi(val());
    else if (a == "--derive-par") {
      std::stringstream ss(val());
      for (std::string tok; std::getline(ss, tok, ',');) derive_par.push_back((float)atof(tok.c_str()));
    }
    else if (a == "--derive-linear") derive_linear_file = val();
    else if (a == "--derived-summary") derived_summary_file = val();
    else if (a == "--derived-rank-summary") derived_rank_summary_file = val();
    else if (a == "--derived-covariance") derived_covariance_file = val();
    else if (a == "--density") density_file = val();
    else if (a == "--derived-density") derived_density_file = val();
    else if (a == "--density-n") density_spec.n = atoi(val());
    else if (a == "--density-clip") {
      if (sscanf(val(), "%lf,%lf", &density_spec.clip_lo, &density_spec.clip_hi) != 2) {
        std::cerr << "--density-clip takes QLO,QHI\n";
        return 2;
      }
    }
    else if (a == "--profile") profile_files.curves = val();
    else if (a == "--profile-intervals") profile_files.intervals = val();
    else if (a == "--profile-n") profile_files.spec.n = atoi(val());
    else if (a == "--profile2d") profile_files.pairs = val();
    else if (a == "--profile2d-n") profile_files.spec2.g = atoi(val());
    else if (a == "--profile-path") {
      const char *v = val();
      const char *comma = strchr(v, ',');
      if (!comma || comma == v || !comma[1]) {
        std::cerr << "--profile-path takes C,FILE\n";
        return 2;
      }
      profile_files.path_col = atoi(v);
      profile_files.path = comma + 1;
    }
    else if (a == "--profile-levels") {
      for (const char *v = val(); *v;) {
        char *end;
        profile_files.levels.push_back(strtod(v, &end));
        if (end == v || (*end && *end != ',')) {
          std::cerr << "--profile-levels takes p1,p2,...\n";
          return 2;
        }
        v = *end ? end + 1 : end;
      }
    }
    else if (a == "--profile-clip") {
      if (sscanf(val(), "%lf,%lf", &profile_files.spec.clip_lo, &profile_files.spec.clip_hi) != 2) {
        std::cerr << "--profile-clip takes QLO,QHI\n";
        return 2;
      }
    }
    else if (a == "--profile2d-pairs") {
      for (const char *v = val(); *v;) {
        int pa, pb, used = 0;
        if (sscanf(v, "%d:%d%n", &pa, &pb, &used) != 2 || (v[used] && v[used] != ',')) {
          std::cerr << "--profile2d-pairs takes a:b,c:d,...\n";
          return 2;
        }
        profile_files.pair_list.push_back(pa);
        profile_files.pair_list.push_back(pb);
        v += used + (v[used] ? 1 : 0);
      }
    }
    else if (a == "--density2d") density2d_file = val();
    else if (a == "--derived-density2d") derived_density2d_file = val();
    else if (a == "--density2d-n") density2d_spec.g = atoi(val());
    else if (a == "--density2d-pairs") {
      std::stringstream ss(val());
      for (std::string tok; std::getline(ss, tok, ',');) {
        int pa, pb;
        if (sscanf(tok.c_str(), "%d:%d", &pa, &pb) != 2) {
          std::cerr << "--density2d-pairs takes a:b,c:d,...\n";
          return 2;
        }
        density2d_pairs.push_back(pa);
        density2d_pairs.push_back(pb);
      }
    }
    else if (a == "--clip") {
      if (sscanf(val(), "%lf,%lf", &clip_spec.qlo, &clip_spec.qhi) != 2) {
        std::cerr << "--clip takes QLO,QHI\n";
        return 2;
      }
    }
    else if (a == "--clip-ll-hi") clip_spec.ll_hi = atof(val());
    else if (a == "--clip-report") clip_report_file = val();
    else if (a == "--clipped") clipped_file = val();
    else if (a == "--clipped-density") clipped_density_file = val();
    else if (a == "--clip-nc") clip_nc = atoi(val());
    else if (a == "--chain-table") chain_table_file = val();
    else if (a == "--chain-keep") {
      if (sscanf(val(), "%lf,%lld,%lld", &chain_rule.z, &chain_rule.min_moves, &chain_rule.max_stay) < 1) {
        std::cerr << "--chain-keep takes Z[,MINMOVES[,MAXSTAY]]\n";
        return 2;
      }
    }
    else if (a == "--kept-chains") kept_chains_file = val();
    else if (a == "--step-table") step_table_file = val();
    else if (a == "--compare") compare_file = val();
    else if (a == "--compare-to") compare_to_file = val();
    else if (a == "--compare-nc") compare_nc = atoi(val());
    else if (a == "--compare-iid") compare_iid = true;
    else if (a == "--compare-halves") compare_halves_file = val();
    else if (a == "--mutual-info") mutinfo_file = val();
    else if (a == "--mi-n" || a == "--mi-k" || a == "--mi-perm") {
      (a == "--mi-n" ? mutinfo_spec.n : a == "--mi-k" ? mutinfo_spec.k : mutinfo_spec.nperm) = atoi(val());
      mutinfo_opts = true;
    } else if (a == "--mi-seed") {
      mutinfo_spec.seed = (uint32_t)strtoul(val(), 0, 10);
      mutinfo_opts = true;
    } else if (a == "--mi-with-ll" || a == "--mi-raw") {
      mutinfo_spec.flags |= a == "--mi-raw" ? MCX_MUTINFO_RAW : MCX_MUTINFO_WITH_LL;
      mutinfo_opts = true;
    } else if (a == "--mi-pairs") {
      for (const char *v = val(); *v;) {
        int pa, pb, used = 0;
        if (sscanf(v, "%d:%d%n", &pa, &pb, &used) != 2 || (v[used] && v[used] != ',')) {
          std::cerr << "--mi-pairs takes a:b,c:d,...\n";
          return 2;
        }
        mutinfo_pairs.push_back(pa);
        mutinfo_pairs.push_back(pb);
        v += used + (v[used] ? 1 : 0);
      }
      mutinfo_opts = true;
    }
    else if (a == "--energy") energy_file = val();
    else if (a == "--energy-halves") energy_halves_file = val();
    else if (a == "--energy-n") {
      const char *v = val();
      const char *comma = strchr(v, ',');
      energy_spec.n_a = atoi(v);
      energy_spec.n_b = comma ? atoi(comma + 1) : energy_spec.n_a;
      energy_opts = true;
    } else if (a == "--energy-perm") {
      energy_spec.nperm = atoi(val());
      energy_opts = true;
    } else if (a == "--energy-seed") {
      energy_spec.seed = (uint32_t)strtoul(val(), 0, 10);
      energy_opts = true;
    } else if (a == "--energy-with-ll") {
      energy_spec.flags |= MCX_ENERGY_WITH_LL;
      energy_opts = true;
    } else if (a == "--energy-raw") {
      energy_spec.flags |= MCX_ENERGY_RAW;
      energy_opts = true;
    }
    else if (a == "--reweight") reweight_file = val();
    else if (a == "--reweight-temper") { reweight_source.temper = true; reweight_source.beta = atof(val()); }
    else if (a == "--reweight-source") reweight_source.source_file = val();
    else if (a == "--reweight-logw") reweight_source.logw_file = val();
    else if (a == "--resampled") resampled_file = val();
    else if (a == "--resampled-density") resampled_density_file = val();
    else if (a == "--resample-n") resample_n = atoll(val());
    else if (a == "--resample-seed") resample_seed = (unsigned)strtoul(val(), 0, 10);
    else if (a == "--intervals") intervals_file = val();
    else if (a == "--evidence") evidence.file = val();
    else if (a == "--evidence-draws") { evidence.ndraw = atoll(val()); evidence.any_option = true; }
    else if (a == "--evidence-seed") { evidence.seed = (unsigned)strtoul(val(), 0, 10); evidence.any_option = true; }
    else if (a == "--evidence-fit-steps") { evidence.fit_steps = atoi(val()); evidence.any_option = true; }
    else if (a == "--evidence-modes") { evidence.modes_k = atoi(val()); evidence.any_option = true; }
    else if (a == "--evidence-scale") { evidence.scale = atof(val()); evidence.any_option = true; }
    else if (a == "--modes") modes_files.modes = val();
    else if (a == "--modes-k") modes_spec.k = atoi(val());
    else if (a == "--modes-seed") modes_spec.seed = (uint32_t)strtoul(val(), 0, 10);
    else if (a == "--modes-iter") modes_spec.max_iter = atoi(val());
    else if (a == "--modes-raw") modes_spec.scale = 0;
    else if (a == "--modes-centres") modes_files.centres = val();
    else if (a == "--mode-weights") modes_files.weights = val();
    else if (a == "--mode-chains") modes_files.chains = val();
    else if (a == "--mode-occupancy") modes_files.occupancy = val();
    else if (a == "--mode-rows" || a == "--mode-summary") {
      const char *v = val(), *comma = strchr(v, ',');
      if (!comma || comma == v || !comma[1]) {
        std::cerr << a << " takes K,FILE\n";
        return 2;
      }
      (a == "--mode-rows" ? modes_files.rows_k : modes_files.summary_k) = atoi(v);
      (a == "--mode-rows" ? modes_files.rows : modes_files.summary) = comma + 1;
    }
    else if (a == "--mess") mess_file = val();
    else if (a == "--mess-max-lag") mess_max_lag = atoi(val());
    else if (a == "--mess-with-ll") mess_with_ll = true;
    else if (a == "--ccf") ccf_file = val();
    else if (a == "--ccf-lags") ccf_lags = atoi(val());
    else if (a == "--hdi" || a == "--interval-probs") {
      std::vector<double> &list = a == "--hdi" ? hdi_mass : interval_probs;
      list.clear();
      std::stringstream ss(val());
      for (std::string tok; std::getline(ss, tok, ',');) list.push_back(atof(tok.c_str()));
    }
    else if (a == "--step-probs") {
      step_probs.clear();
      std::stringstream ss(val());
      for (std::string tok; std::getline(ss, tok, ',');) step_probs.push_back(atof(tok.c_str()));
    }
    else if (a == "--settle") {
      settle = true;
      if (sscanf(val(), "%lf,%lf,%lf", &step_rule.tol_mean, &step_rule.tol_sd, &step_rule.ref_frac) < 1) {
        std::cerr << "--settle takes TOLM[,TOLS[,REF]]\n";
        return 2;
      }
    }
    else if (a == "--kept-summary") kept_summary_file = val();
    else if (a == "--draws") draws_file = val();
    else if (a == "--ndraw") ndraw = atoll(val());
    else if (a == "--draw-seed") draw_seed = (unsigned)strtoul(val(), 0, 10);
    else { std::cerr << "unknown option " << a << "\n"; return 2; }
  }
  profile_files.spec2.clip_lo = profile_files.spec.clip_lo;  // --profile-clip and --profile-levels apply to both
  profile_files.spec2.clip_hi = profile_files.spec.clip_hi;
  if (!profile_files.levels.empty()) {
    profile_files.spec.nlevels = profile_files.spec2.nlevels = (int)profile_files.levels.size();
    profile_files.spec.levels = profile_files.spec2.levels = profile_files.levels.data();
  }
  if (!profile_files.pair_list.empty()) {
    profile_files.spec2.npairs = (int)(profile_files.pair_list.size() / 2);
    profile_files.spec2.pairs = profile_files.pair_list.data();
  }
  density2d_spec.clip_lo = density_spec.clip_lo;  // --density-clip applies to both
  density2d_spec.clip_hi = density_spec.clip_hi;
  if (!density2d_pairs.empty()) {
    density2d_spec.npairs = (int)(density2d_pairs.size() / 2);
    density2d_spec.pairs = density2d_pairs.data();
  }
  MPI_Init(&argc, &argv);
  int size, rank;
  MPI_Comm_size(MPI_COMM_WORLD, &size);
  MPI_Comm_rank(MPI_COMM_WORLD, &rank);
  if (run_only.empty() && evidence.file.empty()) run_only = func_flag;
  if (!read_file.empty() && (!run_only.empty() || !nc_given || size > 1)) {
    if (rank == 0) {
      if (!run_only.empty()) std::cerr << "--read parses a file, there is no run: not with " << run_only << "\n";
      else std::cerr << "--read needs --nc, the chains of the run that wrote the file, and a single rank\n";
    }
    MPI_Finalize();
    return 2;
  }
  if (read_file.empty() && (read_skip != 0 || read_rows != -1)) {
    if (rank == 0) std::cerr << "--read-skip and --read-rows belong to --read FILE\n";
    MPI_Finalize();
    return 2;
  }
  if (!summary_file.empty() && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--summary needs the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  if (!rank_summary_file.empty() && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--rank-summary needs the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  if ((!covariance_file.empty() || !proposal_file.empty()) && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--covariance / --proposal need the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  if (profile_files.any() && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--profile, --profile-intervals, --profile-path and --profile2d need the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  if (!density2d_file.empty() && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--density2d needs the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  if (!density_file.empty() && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--density needs the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  const bool want_clip = !clip_report_file.empty() || !clipped_file.empty() || !clipped_density_file.empty();
  if (want_clip && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--clip-report, --clipped and --clipped-density need the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  const bool want_chains = !chain_table_file.empty() || !kept_chains_file.empty() || !kept_summary_file.empty();
  if (want_chains && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--chain-table, --kept-chains and --kept-summary need the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  if (!intervals_file.empty() && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--intervals needs the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  if ((!mess_file.empty() || !ccf_file.empty()) && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--mess and --ccf need the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  if (modes_files.any() && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--modes and the --mode-* files need the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  if (!evidence.file.empty() && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--evidence needs the rows on the host of a single rank: not with " << (stream_text ? "--stream-text" : "more than one rank")
                << "\n";
    MPI_Finalize();
    return 2;
  }
  if (evidence.file.empty() && evidence.any_option) {
    if (rank == 0) std::cerr << "--evidence-draws, --evidence-seed, --evidence-fit-steps, --evidence-modes and --evidence-scale belong to --evidence FILE\n";
    MPI_Finalize();
    return 2;
  }
  if (!evidence.file.empty() && (evidence.ndraw < 0 || evidence.fit_steps < -1 || evidence.modes_k < 0)) {
    if (rank == 0) std::cerr << "--evidence-draws, --evidence-fit-steps and --evidence-modes take numbers that are not negative\n";
    MPI_Finalize();
    return 2;
  }
  if (modes_files.any() && modes_spec.k < 1) {
    if (rank == 0) std::cerr << "--modes and the --mode-* files need --modes-k K with K >= 1\n";
    MPI_Finalize();
    return 2;
  }
  if (!ccf_file.empty() && ccf_lags < 1) {
    if (rank == 0) std::cerr << "--ccf needs --ccf-lags L with L >= 1\n";
    MPI_Finalize();
    return 2;
  }
  if (settle && step_table_file.empty()) {
    if (rank == 0) std::cerr << "--settle writes into the file of --step-table: give one\n";
    MPI_Finalize();
    return 2;
  }
  if (!step_table_file.empty() && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--step-table needs the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  const bool want_compare = !compare_file.empty() || !compare_halves_file.empty();
  const bool want_energy = !energy_file.empty() || !energy_halves_file.empty();
  if ((compare_file.empty() && energy_file.empty()) != compare_to_file.empty() || (compare_nc != 0 && compare_to_file.empty()) ||
      compare_nc < 0 || (compare_iid && !want_compare)) {
    if (rank == 0)
      std::cerr << "--compare FILE (or --energy FILE) and --compare-to OTHER go together; --compare-nc belongs to them, --compare-iid "
                   "to --compare or to --compare-halves\n";
    MPI_Finalize();
    return 2;
  }
  if (energy_opts && !want_energy) {
    if (rank == 0) std::cerr << "--energy-n, --energy-perm, --energy-seed, --energy-with-ll and --energy-raw belong to --energy or --energy-halves\n";
    MPI_Finalize();
    return 2;
  }
  if (mutinfo_opts && mutinfo_file.empty()) {
    if (rank == 0) std::cerr << "--mi-n, --mi-k, --mi-perm, --mi-seed, --mi-pairs, --mi-with-ll and --mi-raw belong to --mutual-info\n";
    MPI_Finalize();
    return 2;
  }
  if (!mutinfo_file.empty() && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--mutual-info needs the rows on the host of a single rank: not with " << (stream_text ? "--stream-text" : "more than one rank")
                << "\n";
    MPI_Finalize();
    return 2;
  }
  if (!mutinfo_pairs.empty()) {
    mutinfo_spec.npairs = (int)(mutinfo_pairs.size() / 2);
    mutinfo_spec.pairs = mutinfo_pairs.data();
  }
  if (want_energy && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--energy and --energy-halves need the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  if (want_compare && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--compare and --compare-halves need the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  const bool want_resampled = !resampled_file.empty() || !resampled_density_file.empty();
  const bool want_reweight = !reweight_file.empty() || want_resampled;
  const int reweight_sources = (reweight_source.temper ? 1 : 0) + (reweight_source.source_file.empty() ? 0 : 1) + (reweight_source.logw_file.empty() ? 0 : 1);
  if (want_reweight != (reweight_sources == 1) || reweight_sources > 1 || want_resampled != (resample_n > 0)) {
    if (rank == 0)
      std::cerr << "--reweight, --resampled and --resampled-density need exactly one of --reweight-temper BETA, --reweight-source FILE and "
                   "--reweight-logw FILE, and the other way round; --resample-n K (K >= 1) goes with the two --resampled files\n";
    MPI_Finalize();
    return 2;
  }
  if (want_reweight && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--reweight and --resampled need the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  const bool want_derived = !derived_summary_file.empty() || !derived_rank_summary_file.empty() || !derived_covariance_file.empty() ||
                            !derived_density_file.empty() || !derived_density2d_file.empty();
  const bool have_derive = !derive_source_file.empty() || !derive_linear_file.empty();
  if ((want_derived || !draws_file.empty()) && (stream_text || size > 1)) {
    if (rank == 0)
      std::cerr << "--derived-* and --draws need the rows on the host of a single rank: not with "
                << (stream_text ? "--stream-text" : "more than one rank") << "\n";
    MPI_Finalize();
    return 2;
  }
  if (want_derived != have_derive || (!derive_source_file.empty() && !derive_linear_file.empty())) {
    if (rank == 0) std::cerr << "--derived-* files need one of --derive-source and --derive-linear, and the other way round\n";
    MPI_Finalize();
    return 2;
  }

  // --read: the file's rows, parsed on the GPU, before MCout learns its width
  std::vector<float> file_rows;
  if (!read_file.empty()) {
    mcx_text_spec tspec = {np_given ? np + 1 : 0, nc, read_skip, read_rows, 0};
    mcx_text_report trep;
    mcx_store *ts = 0;
    if (mcx_file_store(read_file.c_str(), &tspec, &ts, &trep) != MCX_OK) {
      std::cerr << "--read " << read_file << ": " << mcx_last_error() << "\n";
      MPI_Finalize();
      return 2;
    }
    np = trep.ncol - 1;
    nsamp = (int)(trep.nrows / nc);
    nburn = 0;
    file_rows.resize((size_t)trep.nrows * (size_t)trep.ncol);
    const int rc = mcx_store_copy(ts, 0, nsamp, file_rows.data());
    mcx_store_destroy(ts);
    if (rc != MCX_OK) {
      std::cerr << "--read " << read_file << ": " << mcx_last_error() << "\n";
      MPI_Finalize();
      return 2;
    }
    std::cerr << "read " << trep.nrows << " rows of " << trep.ncol << " columns (" << nsamp << " steps of " << nc << " chains) from "
              << trep.nlines << " lines in " << trep.npieces << " pieces, " << trep.nfallback << " tokens through strtof\n";
  }

  VLFunc *L = 0;
  std::vector<float> means, w;
  try {
    if (!read_file.empty() && evidence.file.empty()) L = 0;  // (no run: no likelihood unless --evidence evaluates one)
    else if (!func_source.empty()) {
      FILE *f = fopen(func_source.c_str(), "rb");
      if (!f) { std::cerr << "cannot read " << func_source << "\n"; return 2; }
      std::string text;
      char buf[4096];
      for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, k);
      fclose(f);
      func = "source:" + func_source;
      L = new SourceVLFunc(np, text.c_str(), user_par.empty() ? 0 : user_par.data(), (int)user_par.size());
    } else
    if (func == "rosen1") L = new Rosenbrock1(np);
    else if (func == "rosen2") L = new Rosenbrock2(np);
    else if (func == "rosen2fixed") L = new Rosenbrock2Fixed(np);  // flagged variant, not reference behaviour
    else if (func == "gauss") L = new Gaussian(np);
    else if (func == "dgauss") { np = 2; L = new DualGaussian(5.0f); }
    else if (func == "mix") {  // means 5k/(K-1) * 1, weights (5,1,...,1)
      means.resize((size_t)ncomp * np);
      w.assign(ncomp, 1.0f);
      w[0] = 5.0f;
      for (int k = 0; k < ncomp; ++k)
        for (int i = 0; i < np; ++i) means[(size_t)k * np + i] = 5.0f * k / (ncomp > 1 ? ncomp - 1 : 1);
      L = new GaussianMixture(np, ncomp, means.data(), w.data());
    } else { std::cerr << "unknown --func " << func << "\n"; return 2; }
  } catch (const char *msg) {
    std::cerr << msg << "\n";
    return 2;
  }

  std::ostringstream sink;
  MCout rslts(np, (quiet || iter) ? static_cast<std::ostream *>(&sink) : &std::cout, MPI_COMM_WORLD);
  rslts.binary(binary);
  rslts.text_only(stream_text && !binary && !iter);
  if (!out_file.empty() && !rslts.text_file(out_file.c_str())) {
    std::cerr << "cannot open " << out_file << "\n";
    MPI_Finalize();
    return 2;
  }
  std::vector<float> incov;
  if (!incov_file.empty() && read_incov(incov_file.c_str(), np, incov) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (!read_file.empty()) {
    rslts.newsamps((int)(file_rows.size() / ((size_t)np + 1)));
    rslts.add_rows(file_rows.data(), file_rows.size() / ((size_t)np + 1));
    std::vector<float>().swap(file_rows);
  }
  std::vector<float> pinit(read_file.empty() ? (size_t)nc * np : 0);
  for (int j = 0; j < nc && read_file.empty(); ++j)
    for (int i = 0; i < np; ++i)
      pinit[(size_t)j * np + i] = (float)(0.5 * std::sin(0.37 * ((double)(rank * nc + j) * np + i)));
  if (read_file.empty()) try {
    MCPar mcpar(np, nc, size, rank, pl, 0.2f, 0.5f, 0.2f, 1.5f, sync);
    auto t0 = std::chrono::steady_clock::now();
    mcpar.run(nsamp, nburn, pinit.data(), *L, rslts, incov.empty() ? 0 : incov.data());
    double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (iter && !quiet) {  // (the numbers through fmtg6 like MCout::output: the same characters as `cout << float`)
      std::vector<char> line((size_t)(np + 1) * 18 + 32);
      for (int r = 0; r < rslts.size(); ++r) {
        char *q = line.data() + snprintf(line.data(), 16, "%d  ", r / nc);
        const float *p = rslts.getpset(r);
        for (int j = 0; j < np + 1; ++j) {
          q = fmtg6::append(q, p[j]);
          *q++ = ' ';
          *q++ = ' ';
        }
        *q++ = '\n';
        std::cout.write(line.data(), q - line.data());
      }
    }
    if (rank == 0)
      std::cerr << "chains " << nc << " x np " << np << "  burn " << nburn << " + samples " << nsamp
                << ": accept rate (main) " << (double)mcpar.naccept_main() / ((double)nc * nsamp)
                << ", remote passes " << mcpar.remote_passes() << ", " << (double)nc * (nburn + nsamp) / dt
                << " chain-steps/s incl. output, exchange: " << mcpar.exchange_backend() << "\n";
  } catch (const char *msg) {
    std::cerr << msg << "\n";
    return 2;
  }
  rslts.text_file(0);
  if (!summary_file.empty() && write_summary(summary_file.c_str(), rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (!rank_summary_file.empty() && write_rank_summary(rank_summary_file.c_str(), rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if ((!covariance_file.empty() || !proposal_file.empty()) &&
      write_covariance(covariance_file.empty() ? 0 : covariance_file.c_str(), proposal_file.empty() ? 0 : proposal_file.c_str(),
                       rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (!density_file.empty() && write_density(density_file.c_str(), density_spec, rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (!density2d_file.empty() && write_density2d(density2d_file.c_str(), density2d_spec, rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (profile_files.any1() && write_profile(profile_files, rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (!profile_files.pairs.empty() && write_profile2d(profile_files, rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (want_clip && write_clip(clip_spec, clip_report_file.empty() ? 0 : clip_report_file.c_str(),
                              clipped_file.empty() ? 0 : clipped_file.c_str(),
                              clipped_density_file.empty() ? 0 : clipped_density_file.c_str(), clip_nc, density_spec, rslts, nsamp, nc,
                              np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (want_chains && write_chains(chain_rule, chain_table_file.empty() ? 0 : chain_table_file.c_str(),
                                  kept_chains_file.empty() ? 0 : kept_chains_file.c_str(),
                                  kept_summary_file.empty() ? 0 : kept_summary_file.c_str(), rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (!intervals_file.empty() && write_intervals(intervals_file.c_str(), hdi_mass, interval_probs, rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if ((!mess_file.empty() || !ccf_file.empty()) &&
      write_lagcov(mess_file.empty() ? 0 : mess_file.c_str(), ccf_file.empty() ? 0 : ccf_file.c_str(), mess_max_lag, mess_with_ll, ccf_lags,
                   rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (!evidence.file.empty() && write_evidence(evidence, L, rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (modes_files.any() && write_modes(modes_files, modes_spec, rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (!step_table_file.empty() && write_steps(step_table_file.c_str(), step_probs, settle ? &step_rule : 0, rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (want_compare && write_compare(compare_file.empty() ? 0 : compare_file.c_str(), compare_to_file.c_str(), compare_nc ? compare_nc : nc,
                                    compare_iid, compare_halves_file.empty() ? 0 : compare_halves_file.c_str(), rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (want_energy && write_energy(energy_file.empty() ? 0 : energy_file.c_str(), compare_to_file.c_str(), compare_nc ? compare_nc : nc,
                                  energy_spec, energy_halves_file.empty() ? 0 : energy_halves_file.c_str(), rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (!mutinfo_file.empty() && write_mutinfo(mutinfo_file.c_str(), mutinfo_spec, rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (want_derived) {
    mcx_derive spec = {MCX_DERIVE_LINEAR, derive_nout, 0, 0, 0};
    std::string text;
    if (!derive_linear_file.empty()) {
      if (read_linear(derive_linear_file.c_str(), np, derive_par, &spec.nout) != 0) {
        MPI_Finalize();
        return 2;
      }
    } else {
      FILE *f = fopen(derive_source_file.c_str(), "rb");
      if (!f) {
        std::cerr << "cannot read " << derive_source_file << "\n";
        MPI_Finalize();
        return 2;
      }
      char buf[4096];
      for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, k);
      fclose(f);
      spec.kind = MCX_DERIVE_SOURCE;
      spec.source = text.c_str();
    }
    spec.npar = (int)derive_par.size();
    spec.par = derive_par.empty() ? 0 : derive_par.data();
    if (write_derived(spec, derived_summary_file.empty() ? 0 : derived_summary_file.c_str(),
                      derived_rank_summary_file.empty() ? 0 : derived_rank_summary_file.c_str(),
                      derived_covariance_file.empty() ? 0 : derived_covariance_file.c_str(),
                      derived_density_file.empty() ? 0 : derived_density_file.c_str(), density_spec,
                      derived_density2d_file.empty() ? 0 : derived_density2d_file.c_str(), density2d_spec, rslts, nsamp, nc, np) != 0) {
      MPI_Finalize();
      return 2;
    }
  }
  if (want_reweight && write_reweight(reweight_source, derive_par, reweight_file.empty() ? 0 : reweight_file.c_str(),
                                      resampled_file.empty() ? 0 : resampled_file.c_str(),
                                      resampled_density_file.empty() ? 0 : resampled_density_file.c_str(), resample_n, resample_seed,
                                      density_spec, rslts, nsamp, nc, np) != 0) {
    MPI_Finalize();
    return 2;
  }
  if (!draws_file.empty() && write_draws(draws_file.c_str(), rslts, np, ndraw, draw_seed) != 0) {
    MPI_Finalize();
    return 2;
  }
  float lmax;
  const std::vector<float> &pmax = rslts.maxlike(&lmax);
  if (rank == 0) {
    std::cerr << "max likelihood value: " << lmax << "\n";
    for (size_t i = 0; i < pmax.size() && i < 8; ++i) std::cerr << pmax[i] << "  ";
    std::cerr << "\n";
  }
  delete L;
  MPI_Finalize();
  return 0;
}
