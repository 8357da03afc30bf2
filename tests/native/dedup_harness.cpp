// Test-only host build of the message-group path (GBLS_INIT_DEDUP): the engine's g1s addition
// in both arithmetic layers, and a sequential emulation of the grouped pipeline -- the plan of
// gbls_dedup.h, the group sums k_g1s_msgsum forms, then the engine's Miller product and final
// verdict as host_harness.cpp's pipeline runs them.  Built on host_harness.cpp (its static
// helpers), as a shared object of its own; not part of the product.
#include "host_harness.cpp"

#include "../../grandine_amd/csrc/gbls_dedup.h"

static void h_sum_add(g1s &acc, const g1s &v, int layer) {
  if (layer == 0) {
    g1s_add(acc, acc, v);
    return;
  }
  r28::g1h28 a, b;  // one addition as the radix-2^28 kernel does it, through the engine form
  r28::g1h28_load(a, acc);
  r28::g1h28_load(b, v);
  r28::g1h28_add(a, a, b);
  r28::g1h28_store(acc, a);
}

extern "C" {

// out = a + b for line-evaluation points (x, y, c; 3 x 48 bytes, Montgomery form).
// layer 0: bls_pairing.h g1s_add; 1: bls_curve28.h g1h28_add between load and store
void h_g1s_add(const uint8_t *a144, const uint8_t *b144, uint8_t *out144, int layer) {
  g1s a, b;
  std::memcpy(&a, a144, 144);
  std::memcpy(&b, b144, 144);
  h_sum_add(a, b, layer);
  std::memcpy(out144, &a, 144);
}

// a chain in the radix-2^28 layer without leaving it (the kernel's accumulator): sum of n points
void h_g1s_sum28(const uint8_t *pts144, uint32_t n, uint8_t *out144) {
  r28::g1h28 acc, v;
  r28::g1h28_set_inf(acc);
  for (uint32_t i = 0; i < n; i++) {
    g1s p;
    std::memcpy(&p, pts144 + 144 * (size_t)i, 144);
    r28::g1h28_load(v, p);
    r28::g1h28_add(acc, acc, v);
  }
  g1s o;
  r28::g1h28_store(o, acc);
  std::memcpy(out144, &o, 144);
}

// The grouped pipeline of pipeline_partials with a plan: per segment, one hash_to_G2, one set of
// lines and one Miller pair per message group, the pair's G1 point the sum of the members'
// r_i pk_i; S and every per-set rejection stay per set.  Returns the number of groups.
int h_multi_verify_dedup(const uint8_t *msgs32, const uint8_t *sigs192, const uint8_t *pks96,
                         const uint64_t *rands, uint32_t n, const uint32_t *seg_off, uint32_t nseg, int layer,
                         int32_t *verdicts) {
  dedup::Plan pl;
  dedup::build(pl, msgs32, n, seg_off, nseg);
  const uint8_t *um = pl.has_duplicates() ? pl.msgs.data() : msgs32;  // U == n: groups are the sets
  for (uint32_t s = 0; s < nseg; s++) {
    const uint32_t g0 = pl.grp_seg_off[s], g1 = pl.grp_seg_off[s + 1];
    const uint32_t np = g1 - g0 + 1;
    std::vector<uint32_t> L((size_t)np * ML_EVENTS * 72);
    std::vector<g1s> P(np);
    g2j S;
    jac_set_inf(S);
    int err = seg_off[s + 1] == seg_off[s];
    for (uint32_t g = g0; g < g1; g++) {
      const uint8_t *m = um + 32 * (size_t)(pl.has_duplicates() ? g : pl.grp_set[pl.grp_off[g]]);
      fp2 u[2];
      hash_to_field_g2(u, m, 32, dst_ref{POP, 43});
      g2j q0, q1, h;
      map_to_g2(q0, u[0]);
      map_to_g2(q1, u[1]);
      jac_add(q0, q0, q1);
      clear_cofactor_g2(h, q0);
      g2a H;
      jac_to_aff(H, h);
      lines_of(L.data(), np, g - g0, H);
      g1s acc;
      fp_zero(acc.x);
      fp_zero(acc.y);
      fp_zero(acc.c);
      for (uint32_t j = pl.grp_off[g]; j < pl.grp_off[g + 1]; j++) {
        const uint32_t i = pl.grp_set[j];
        g1a pk;
        g2a sig;
        std::memcpy(&pk, pks96 + 96 * (size_t)i, 96);
        std::memcpy(&sig, sigs192 + 192 * (size_t)i, 192);
        g1j t;
        mul_u64(t, pk, rands[i]);  // k_mv_g1mul, into the per-set workspace
        g1s pi;
        g1s_from_jac(pi, t);
        h_sum_add(acc, pi, layer);  // k_g1s_msgsum
        err |= aff_is_inf(pk) || rands[i] == 0;
        g2j R;
        mul_u64(R, sig, rands[i]);
        jac_add(S, S, R);
      }
      P[g - g0] = acc;
    }
    fp_set(P[np - 1].x, k::G1X_M);
    fp_set(P[np - 1].y, k::G1NEGY_M);
    fp_one(P[np - 1].c);
    g2a Sa;
    jac_to_aff(Sa, S);
    lines_of(L.data(), np, np - 1, Sa);
    fp12 f;
    for (int e = 0; e < ML_EVENTS; e++) {
      fp12 M;
      fp12_one(M);
      for (uint32_t j = 0; j < np; j++) {
        fp2 L0, L2, L3;
        sp034 sp;
        line_get(L.data(), np, j, e, L0, L2, L3);
        line_eval_s(sp, L0, L2, L3, P[j]);
        fp12_mul_034(M, M, sp);
      }
      if (e == 0) {
        f = M;
      } else {
        if (ev_is_dbl(e)) fp12_sqr(f, f);
        fp12_mul(f, f, M);
      }
    }
    fp12_conj(f, f);
    verdicts[s] = (!err && w12_final_verdict_host(f)) ? ST_SUCCESS : ST_VERIFY_FAIL;
  }
  return (int)pl.ngroups;
}

}  // extern "C"
