/*
 * bh_tidal_ref.c — the reference's octree walked from arbitrary points, returning the TIDAL TENSOR next to the acceleration.  TEST
 * INFRASTRUCTURE ONLY (tests/bh_tidal_ref.py builds and loads it; nothing under parallelnbody_amd/ links it): the yardstick of
 * nbody_tidal_at, nbody_get_tidal and nbody_tidal_time at theta > 0.
 *
 * The tree is bh_ref_tree.h's, the walk and the acceleration those of tests/cpp/bh_pot_ref.c (tests/test_bh_tidal_ref.py pins the
 * acceleration to it in every byte).  The tensor is build-defined (the reference computes none): in the same walk an accepted node (CoM c,
 * mass M) adds, every operation one correctly rounded operation,
 *         e_a = p_a - c_a                                   (fp32, the differences d2 was made of)
 *         ds  = sqrtf(d2 + eps2)                            (fp32, the add one fp32 add)
 *         u = 1.0 / (double)ds;  u2 = u * u;  gm = g * (double)M
 *         q3 = (gm * u) * u2;  h = (3.0 * q3) * u2
 *         hx = h * ex;  hy = h * ey;  hz = h * ez           (the doubles of the fp32 e)
 *         Sxx += hx * ex;  Sxy += hx * ey;  Sxz += hx * ez;  Syy += hy * ey;  Syz += hy * ez;  Szz += hz * ez;  Q += q3
 * to seven double sums in walk order; the result is t64 = (Sxx - Q, Syy - Q, Szz - Q, Sxy, Sxz, Syz) and t = (float)t64.
 * Compile with -ffp-contract=off and without -ffast-math.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "bh_ref_tree.h"

#define API __attribute__((visibility("default")))

/* s: Sxx, Syy, Szz, Sxy, Sxz, Syz, Q */
static void forces(const otree *t, int k, const float pi[3], float theta, double g, float eps2, float acc[3], double s[7]) {
  const onode *nd = &t->nodes[k];
  const int leaf = is_leaf(t, k);
  if (leaf && nd->particle == -1) return;
  const float ex = pi[0] - nd->com[0], ey = pi[1] - nd->com[1], ez = pi[2] - nd->com[2];
  float d2 = ex * ex + ey * ey;
  d2 = d2 + ez * ez;
  const float d = sqrtf(d2);                       /* the walk's decisions: the unsoftened distance */
  if (d == 0.0f) return;
  if (nd->size / d < theta || nd->particle != -1) {
    const float ds2 = d2 + eps2;                   /* the term's: the softened one */
    const float dsf = sqrtf(ds2);
    const double ds = (double)dsf;
    const float sc = (float)(g * (double)nd->total_mass / ((ds * ds) * ds));
    acc[0] = acc[0] + sc * (nd->com[0] - pi[0]);
    acc[1] = acc[1] + sc * (nd->com[1] - pi[1]);
    acc[2] = acc[2] + sc * (nd->com[2] - pi[2]);
    const double u = 1.0 / ds;
    const double u2 = u * u;
    const double gm = g * (double)nd->total_mass;
    const double q3 = (gm * u) * u2;
    const double h = (3.0 * q3) * u2;
    const double dx = (double)ex, dy = (double)ey, dz = (double)ez;
    const double hx = h * dx, hy = h * dy, hz = h * dz;
    s[0] = s[0] + hx * dx; s[3] = s[3] + hx * dy; s[4] = s[4] + hx * dz;
    s[1] = s[1] + hy * dy; s[5] = s[5] + hy * dz;
    s[2] = s[2] + hz * dz;
    s[6] = s[6] + q3;
  } else if (!leaf) {
    for (int i = 0; i < 8; ++i) forces(t, nd->child[i], pi, theta, g, eps2, acc, s);
  }
}

/* CreateOctree (OctreeSearch.cpp:74-89) of the n bodies, then the walk from each of the m points.  acc: m x 3; t64, t: m x 6 each
 * (xx, yy, zz, xy, xz, yz).  Returns 0, 1 past depth 200, 2 out of memory. */
API int bhtidal_walk_f32(int n, const float *pos, const float *mass, const float root_origin[3], float root_size, float theta, double g,
                         float eps2, int div_mode, int m, const float *pts, float *acc, double *t64, float *tf, float root_com_out[3],
                         float *root_mass_out, int *node_count_out) {
  otree t;
  memset(&t, 0, sizeof(t));
  t.pos = pos; t.mass = mass; t.div_mode = div_mode;
  const int root = node_new(&t, root_origin, root_size);
  if (root < 0) return 2;
  for (int i = 0; i < n && !t.overflow; ++i) add(&t, root, i, 0);
  if (t.overflow) { const int e = t.overflow; free(t.nodes); return e; }
  compute_mass(&t, root);
#pragma omp parallel for schedule(dynamic, 256) if (m >= 16384)
  for (int k = 0; k < m; ++k) {
    float a[3] = {0.0f, 0.0f, 0.0f};
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    forces(&t, root, &pts[3 * k], theta, g, eps2, a, s);
    acc[3 * k + 0] = a[0]; acc[3 * k + 1] = a[1]; acc[3 * k + 2] = a[2];
    double *o = &t64[6 * k];
    o[0] = s[0] - s[6]; o[1] = s[1] - s[6]; o[2] = s[2] - s[6];
    o[3] = s[3]; o[4] = s[4]; o[5] = s[5];
    for (int c = 0; c < 6; ++c) tf[6 * k + c] = (float)o[c];
  }
  if (root_com_out) memcpy(root_com_out, t.nodes[root].com, sizeof(float) * 3);
  if (root_mass_out) *root_mass_out = t.nodes[root].total_mass;
  if (node_count_out) *node_count_out = t.count;
  free(t.nodes);
  return 0;
}
