// Node-level arithmetic of the gradient kernels that the host can run too (TC_HD, fastmath.h):
// the Gaussian of a central node with its tails, and the Leauthaud11 family -- the inverse
// stellar-to-halo mass relation, the occupations of a node and their derivatives with respect to
// the eleven parameters (grad.h: kGradParamsLeauthaud11).  grad_kernels.hip.h sums these over the
// nodes of a bin; tc_debug_leauthaud11_node_grad (runtime.cpp) evaluates them for arrays of
// masses without a GPU.
//
// With x = log10 M* + 2 log10 h - logm0, a = 10^(delta x), b = 10^(-gamma x):
//   g(x) = beta x + a / (1 + b),  g' = beta + ln10 a / (1 + b) (delta + gamma b / (1 + b)),
//   g_beta = x,  g_delta = ln10 x a / (1 + b),  g_gamma = ln10 x a b / (1 + b)^2.
// Centrals: x solves g(x) = log10 M_h + log10 h + 1/2 - logm1, so by the implicit function
//   theorem dlog M*/d(logm0, logm1, beta, delta, gamma) = (1, -1, -g_beta, -g_delta, -g_gamma) /
//   g' (the first one plainly 1) at the root; N_cen = (1 + erf y) / 2 with y = (log M* -
//   threshold) / (sqrt 2 scatter) is the Zheng07 central in y: dN_cen/dp = exp(-y^2) /
//   (sqrt(2 pi) scatter) dlog M*/dp and dN_cen/dscatter = -y exp(-y^2) / (sqrt(pi) scatter).
// Knee, once per draw: x_t = threshold + 2 log10 h - logm0, log K = logm1 + g(x_t) - 1/2 -
//   log10 h + log10 h_s - 12, dlog K/d(logm0, logm1, beta, delta, gamma) = (-g'(x_t), 1,
//   g_beta(x_t), g_delta(x_t), g_gamma(x_t)).
// Satellites: u = M h_s, M_sat = 1e12 bsat K^betasat, M_cut = 1e12 bcut K^betacut, N_s =
//   (u / M_sat)^alphasat exp(-M_cut / u); with A = N_s, B = N_s M_cut / u, C = N_s ln(u / M_sat):
//   d/dalphasat = C, d/dbsat = -alphasat A / bsat, d/dbetasat = -alphasat ln10 log K A,
//   d/dbcut = -N_s (1e12 K^betacut) / u (finite at bcut = 0), d/dbetacut = -ln10 log K B, and for
//   each of the five relation parameters dlog K/dp ln10 (-alphasat betasat A - betacut B);
//   with modulate_with_cenocc the product rule with N_cen at the satellites' own node.
#pragma once

#include "fastmath.h"
#include "grad.h"

namespace tc {
namespace grad {

constexpr double kLn10 = 2.302585092994045684;
constexpr double kLog2E = 1.4426950408889634074;
constexpr double kTwoOverSqrtPi = 1.1283791670955125739;
constexpr double kLog2Of10 = 3.32192809488736234787;
constexpr double kLog10Of2 = 0.30102999566398119521;

// N = (1 + erf x) / 2 at x (`inv_sigma` = dx / dlog M) and its derivatives: dn0 = -dN/dlog M =
// -exp(-x^2) inv_sigma / sqrt(pi), dn1 = x dn0.
// erf_gauss_fast counts the Gaussian as zero from |x| = 6 on; the derivative of a draw whose
// every node lies out there is made of exactly these tails, so they are evaluated: exp(-x^2) =
// 2^z with the rounding error of the product z = -x^2 log2 e carried along.
// x_abs, gauss_out: |x| and 2/sqrt(pi) exp(-x^2), for the decorated centrals.
TC_HD void central_node_at(const double* mt, const fm::Consts& k, double x, double inv_sigma,
                           double* n, double* dn0, double* dn1, double* x_abs = nullptr,
                           double* gauss_out = nullptr) {
  double gauss;
  const double e = fm::erf_gauss_fast(mt, k, x, &gauss);
  const double x2 = x * x;
  const double zh = -x2 * kLog2E;
  const double zl = fma(-x2, kLog2E, -zh) - fma(x, x, -x2) * kLog2E;
  const double t = fm::exp2_fast(mt, k, zh, zh > -1000.0);
  const double tail = kTwoOverSqrtPi * fma(t, zl * fm::kLn2, t);
  gauss = fabs(x) < 6.0 ? gauss : tail;
  *n = fma(0.5, e, 0.5);
  *dn0 = -0.5 * gauss * inv_sigma;
  *dn1 = *dn0 * x;
  if (x_abs != nullptr) *x_abs = fabs(x);
  if (gauss_out != nullptr) *gauss_out = gauss;
}

// ---- Leauthaud11 ---------------------------------------------------------------------------------

// Quantities of a node or bin, in row order: the value, then the eleven derivatives in the order
// of the first eleven theta columns.
enum Leauthaud11Quantity {
  kL11Value = 0, kL11LogM0, kL11LogM1, kL11Beta, kL11Delta, kL11Gamma, kL11Scatter,
  kL11AlphaSat, kL11BSat, kL11BetaSat, kL11BCut, kL11BetaCut
};

struct Leauthaud11Draw {
  // the relation (kernels.hip.h: SmhmSetup); offset = log10 h + 1/2 - logm1
  double log_m0, beta, delta, gamma, offset, two_log_h;
  double threshold;
  double inv_width;      // 1 / (sqrt 2 scatter)
  // satellites, as prepare_leauthaud has them: log2(M_sat / h_s), -M_cut log2 e / h_s
  double alphasat, log2_msat, cut;
  double inv_bsat;
  double cut_slope;      // 1e12 K^betacut / h_s: M_cut / (bcut h_s)
  double ln_knee;        // ln10 log K
  double betasat_term;   // -alphasat betasat ln10
  double betacut_term;   // -betacut ln10
  double dlog_knee[5];   // dlog K / d(logm0, logm1, beta, delta, gamma)
};

// a = 10^(delta x), b = 10^(-gamma x) and what the relation and its derivatives are made of
struct SmhmPoint {
  double x, ratio, inv, b, slope;      // ratio = a / (1 + b), inv = 1 / (1 + b), slope = g'
};

TC_HD void smhm_point(const double* mt, const fm::Consts& k, const Leauthaud11Draw& d, double x,
                      SmhmPoint* p) {
  const double a = fm::exp10_fast(mt, k, d.delta * x);
  p->b = fm::exp10_fast(mt, k, -d.gamma * x);
  p->inv = 1.0 / (1.0 + p->b);
  p->ratio = a * p->inv;
  p->slope = fma(kLn10 * p->ratio, fma(d.gamma * p->b, p->inv, d.delta), d.beta);
  p->x = x;
}
TC_HD double smhm_g(const Leauthaud11Draw& d, const SmhmPoint& p) {
  return fma(d.beta, p.x, p.ratio);
}
TC_HD double smhm_g_delta(const SmhmPoint& p) { return kLn10 * p.x * p.ratio; }
TC_HD double smhm_g_gamma(const SmhmPoint& p) { return kLn10 * p.x * p.ratio * (p.b * p.inv); }

// The root x of g(x) = log10 M_h + offset by Newton's method, with the start and the criterion of
// the forward kernels (kernels.hip.h: smhm_log_mstar), but every lane for itself: a lane leaves
// the loop with its own last step, so that a draw's root depends on the draw alone.  `point`: a,
// b and g' of the last iteration, one step (at most 1e-15 max(1, |x|)) before the root: they serve
// the derivatives.  Returns log10 M*.
TC_HD double smhm_root(const double* mt, const fm::Consts& k, const Leauthaud11Draw& d,
                       double log_mh, SmhmPoint* point) {
  const double target = log_mh + d.offset;
  double x = target / d.beta;
  if (target > 0.5) {
    const double alt = fm::log2_fast(mt, k, 2.0 * target) * (kLog10Of2 / d.delta);
    x = alt < x ? alt : x;
  }
  for (int iteration = 0; iteration < 24; ++iteration) {
    smhm_point(mt, k, d, x, point);
    const double step = (smhm_g(d, *point) - target) / point->slope;
    x -= step;
    const double scale = fabs(x) > 1.0 ? fabs(x) : 1.0;
    if (!(fabs(step) > 1e-15 * scale)) break;     // (a NaN lane leaves at once)
  }
  return x + d.log_m0 - d.two_log_h;
}

TC_HD Leauthaud11Draw prepare_leauthaud11(const double* mt, const fm::Consts& k,
                                          const double* th) {
  const double log_m0 = th[0], log_m1 = th[1], beta = th[2], delta = th[3], gamma = th[4];
  const double scatter = th[5], alphasat = th[6], bsat = th[7], betasat = th[8];
  const double bcut = th[9], betacut = th[10], threshold = th[11], h = th[12];
  const double h_sat = th[13];
  const double nan = __builtin_nan("");
  const double log_h = fm::log2_fast(mt, k, h > 1e-300 ? h : 1e-300) * kLog10Of2;
  const double log_hs = fm::log2_fast(mt, k, h_sat > 1e-300 ? h_sat : 1e-300) * kLog10Of2;
  Leauthaud11Draw d;
  d.log_m0 = log_m0;
  d.beta = beta;
  d.delta = delta;
  d.gamma = gamma;
  d.offset = log_h + 0.5 - log_m1;
  d.two_log_h = 2.0 * log_h;
  d.threshold = threshold;
  d.inv_width = 1.0 / (1.41421356237309504880 * scatter);
  // the knee: the forward relation at the threshold, in units of 1e12
  SmhmPoint t;
  smhm_point(mt, k, d, threshold + 2.0 * log_h - log_m0, &t);
  const double log_knee = log_m1 + beta * t.x + t.ratio - 0.5 - log_h + log_hs - 12.0;
  d.dlog_knee[0] = -t.slope;
  d.dlog_knee[1] = 1.0;
  d.dlog_knee[2] = t.x;
  d.dlog_knee[3] = smhm_g_delta(t);
  d.dlog_knee[4] = smhm_g_gamma(t);
  // log2 M_sat and M_cut (bsat <= 0 or bcut < 0 have no real power law: NaN)
  const double log2_msat =
      bsat > 0.0 ? fm::log2_fast(mt, k, bsat) + (12.0 + betasat * log_knee) * kLog2Of10 : nan;
  const double cut_exponent = (12.0 + betacut * log_knee) * kLog2Of10;
  d.alphasat = alphasat;
  d.log2_msat = log2_msat - log_hs * kLog2Of10;
  d.cut_slope = bcut >= 0.0 && cut_exponent == cut_exponent
                    ? fm::exp2_fast(mt, k, cut_exponent) / h_sat
                    : nan;
  d.cut = -(bcut * d.cut_slope) * kLog2E;
  d.inv_bsat = 1.0 / bsat;
  d.ln_knee = kLn10 * log_knee;
  d.betasat_term = -alphasat * betasat * kLn10;
  d.betacut_term = -betacut * kLn10;
  return d;
}

// <N_cen> at a node of log10 mass log_m: out[0] = N_cen, out[1 .. 6] its derivatives with respect
// to logm0, logm1, beta, delta, gamma, scatter (the other five are zero and not written).
// Returns log10 M*.
TC_HD double leauthaud11_central_node(const double* mt, const fm::Consts& k,
                                      const Leauthaud11Draw& d, double log_m, double out[7]) {
  SmhmPoint p;
  const double log_mstar = smhm_root(mt, k, d, log_m, &p);
  const double y = (log_mstar - d.threshold) * d.inv_width;
  double n, dn0, dn1;
  central_node_at(mt, k, y, d.inv_width, &n, &dn0, &dn1);
  n = y != y ? y : n;                     // NaN parameters stay NaN (the table functions clamp)
  const double slope = -dn0;              // dN_cen / dlog M*
  const double per_g = -slope / p.slope;
  out[kL11Value] = n;
  out[kL11LogM0] = slope;
  out[kL11LogM1] = per_g;
  out[kL11Beta] = per_g * p.x;
  out[kL11Delta] = per_g * smhm_g_delta(p);
  out[kL11Gamma] = per_g * smhm_g_gamma(p);
  // dN/dscatter = sqrt 2 dN/d(sqrt 2 scatter)
  out[kL11Scatter] = 1.41421356237309504880 * dn1;
  return log_mstar;
}

// <N_sat> at a node of mass m (log10 mass log_m), out[0 .. 11]: the value and all eleven
// derivatives; with `modulate` times <N_cen> at the same node (cen: leauthaud11_central_node's
// results there), by the product rule.
TC_HD void leauthaud11_satellite_node(const double* mt, const fm::Consts& k,
                                      const Leauthaud11Draw& d, double log_m, double m,
                                      bool modulate, const double cen[7], double out[12]) {
  // (M h_s / M_sat)^alphasat exp(-M_cut / (M h_s)) as one power of two, as the forward kernels
  const double log2_ratio = log_m * kLog2Of10 - d.log2_msat;
  const double inv_m = 1.0 / m;
  const double z = fma(d.alphasat, log2_ratio, d.cut * inv_m);
  double n = fm::exp2_fast(mt, k, z);
  n = z != z ? z : n;                     // NaN parameters stay NaN (exp2_fast clamps)
  const double per_cut = n * (d.cut_slope * inv_m);       // N_s (1e12 K^betacut) / u
  const double b = -d.cut * fm::kLn2 * inv_m * n;         // B = N_s M_cut / u
  const double relation = fma(d.betasat_term, n, d.betacut_term * b);
  out[kL11Value] = n;
#pragma unroll
  for (int p = 0; p < 5; ++p) out[kL11LogM0 + p] = d.dlog_knee[p] * relation;
  out[kL11Scatter] = 0.0;
  out[kL11AlphaSat] = n * fm::ln_from_log2(log2_ratio);
  out[kL11BSat] = -d.alphasat * n * d.inv_bsat;
  out[kL11BetaSat] = -d.alphasat * d.ln_knee * n;
  out[kL11BCut] = -per_cut;
  out[kL11BetaCut] = -d.ln_knee * b;
  if (modulate) {
#pragma unroll
    for (int p = kL11LogM0; p <= kL11Scatter; ++p) out[p] = fma(out[p], cen[0], n * cen[p]);
#pragma unroll
    for (int p = kL11AlphaSat; p <= kL11BetaCut; ++p) out[p] *= cen[0];
    out[kL11Value] = n * cen[0];
  }
}

}  // namespace grad
}  // namespace tc
