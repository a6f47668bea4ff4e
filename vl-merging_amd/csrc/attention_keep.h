// Kept query rows of the fused attention (vlm_attn_desc_t.q_keep0 / q_keep1, include/vlm_hip.h): the caller wants the outputs
// of the first q_keep0 text and the first q_keep1 image QUERY positions of every sample only (keys are never limited).  In
// position space (attention_common.h) that is [0, qt) and [pos1, qe): at most two runs of 128-position tiles (forward, dQ) or of
// 32-position blocks (the streamed side of the fused dK / dV / bias-gradient kernel).  Plain C++ with no device code in it: the
// launchers, the kernels and tests/helpers/attn_keep_check.cpp all read the runs from here.
#pragma once

#ifdef __HIPCC__
#define ATT_KEEP_HD __host__ __device__
#else
#define ATT_KEEP_HD
#endif

struct att_keep_t {
  int qt;  // kept text positions are [0, qt)
  int qe;  // kept image positions are [pos1, qe)
};

// (0, 0) or less means "all"; a limit past its segment is the whole segment
static inline ATT_KEEP_HD bool att_keep_all(int k0, int k1) { return k0 <= 0 && k1 <= 0; }

static inline ATT_KEEP_HD att_keep_t att_keep_limits(int n0, int n1, int pos1, int k0, int k1) {
  att_keep_t k;
  if (att_keep_all(k0, k1)) { k.qt = n0; k.qe = pos1 + n1; return k; }
  k.qt = k0 < 0 ? 0 : (k0 < n0 ? k0 : n0);
  k.qe = pos1 + (k1 < 0 ? 0 : (k1 < n1 ? k1 : n1));
  return k;
}

static inline ATT_KEEP_HD bool att_keep_pos(const att_keep_t& k, int pos1, int p) { return p < k.qt || (p >= pos1 && p < k.qe); }

// The kept units (unit = 128: stationary tiles, unit = 32: streamed blocks) of a part whose positions start at `org` and whose
// FULL range holds `full` units: compact index i stands for unit i (i < na) or i + shift (na <= i < n).  joint: the part holds
// text then image positions from 0 (JOINT mode); otherwise it is one segment (SEPARATE: seg 0 text from 0, seg 1 image from pos1).
struct att_keep_run_t {
  int na, shift, n;
};
static inline ATT_KEEP_HD int att_keep_unit(const att_keep_run_t& r, int i) { return i < r.na ? i : i + r.shift; }
static inline ATT_KEEP_HD bool att_keep_has(const att_keep_run_t& r, int u) {
  return u < r.na || (u >= r.na + r.shift && u < r.n + r.shift);
}
static inline ATT_KEEP_HD att_keep_run_t att_keep_run(int n0, int n1, int pos1, int k0, int k1, bool joint, int seg, int unit,
                                                      int full) {
  att_keep_run_t r;
  if (att_keep_all(k0, k1)) { r.na = full; r.shift = 0; r.n = full; return r; }
  const att_keep_t k = att_keep_limits(n0, n1, pos1, k0, k1);
  const int kt = k.qt, ki = k.qe - pos1;
  if (!joint) {
    r.shift = 0;
    r.na = seg == 0 ? (kt + unit - 1) / unit : 0;
    r.n = seg == 0 ? r.na : (ki + unit - 1) / unit;
    return r;
  }
  r.na = (kt + unit - 1) / unit;
  r.shift = 0;
  r.n = r.na;
  if (ki > 0) {
    int b0 = pos1 / unit;
    const int b1 = (pos1 + ki + unit - 1) / unit;
    if (b0 < r.na) b0 = r.na;
    if (b1 > b0) { r.shift = b0 - r.na; r.n = r.na + (b1 - b0); }
  }
  return r;
}

// The 128-position tiles of a launch in att_span's numbering (SEPARATE: text tiles, then image tiles)
static inline ATT_KEEP_HD att_keep_run_t att_keep_tiles(int n0, int n1, int pos1, int k0, int k1, int separate) {
  const int nt0 = (n0 + 127) / 128, nt1 = (n1 + 127) / 128;
  if (!separate) return att_keep_run(n0, n1, pos1, k0, k1, true, 0, 128, (pos1 + n1 + 127) / 128);
  if (att_keep_all(k0, k1)) { const att_keep_run_t r = {nt0 + nt1, 0, nt0 + nt1}; return r; }
  const att_keep_run_t a = att_keep_run(n0, n1, pos1, k0, k1, false, 0, 128, nt0);
  const att_keep_run_t b = att_keep_run(n0, n1, pos1, k0, k1, false, 1, 128, nt1);
  const att_keep_run_t r = {a.n, nt0 - a.n, a.n + b.n};
  return r;
}

// A kept position of the part (what an unkept query lane reads instead of its own row), or -1 when the part keeps none
static inline ATT_KEEP_HD int att_keep_anchor(const att_keep_t& k, int pos1, int s_lo, int s_hi) {
  if (s_lo < k.qt && s_lo < s_hi) return s_lo;
  const int p = s_lo > pos1 ? s_lo : pos1;
  return (p < k.qe && p < s_hi) ? p : -1;
}
