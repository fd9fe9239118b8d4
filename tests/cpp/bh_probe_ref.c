/*
 * bh_probe_ref.c — the reference's octree walked from points that are NOT bodies.  TEST INFRASTRUCTURE ONLY (tests/bh_probe_ref.py
 * builds and loads it; nothing under parallelnbody_amd/ links it): the yardstick of nbody_field_at and of the tracers at theta > 0.
 *
 * The tree is the one of tests/cpp/bh_softened_ref.c (bh_ref_tree.h):
 *   - Octree::Add (OctreeSearch.h:60-81) with the children's centres in double rounded to fp32, cut off past depth 200;
 *   - ComputeMass (.h:83-97) under both readings of `/=` (div_mode 0: the fp32 reciprocal multiplied, 1: three divisions);
 *   - ComputeForces (.h:99-108) with the cube as (d*d)*d in double and the softened term of include/nbody.h: where the walk goes — the
 *     empty leaf, d == 0, Size / d < Theta, the leaf rule — is decided on the UNSOFTENED d; an accepted node adds
 *         ds2 = d2 + eps2 (one fp32 add), ds = sqrtf(ds2), s = (float)(G * M / ((ds*ds)*ds in double)), term = s * (CoM - Pos).
 * The walk function takes an ARBITRARY point: with the points set to the bodies' own positions it is the walk of every body
 * (tests/test_bh_probe_ref.py pins that to the checker the project already trusts, bit for bit); any other point goes through the
 * very same function.
 * Compile with -ffp-contract=off and without -ffast-math.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "bh_ref_tree.h"

#define API __attribute__((visibility("default")))

static void forces(const otree *t, int k, const float pi[3], float theta, double g, float eps2, float acc[3]) {
  const onode *nd = &t->nodes[k];
  const int leaf = is_leaf(t, k);
  if (leaf && nd->particle == -1) return;
  const float ex = pi[0] - nd->com[0], ey = pi[1] - nd->com[1], ez = pi[2] - nd->com[2];
  float d2 = ex * ex + ey * ey;
  d2 = d2 + ez * ez;
  const float d = sqrtf(d2);                       /* the walk's decisions: the unsoftened distance */
  if (d == 0.0f) return;
  if (nd->size / d < theta || nd->particle != -1) {
    const float ds2 = d2 + eps2;                   /* the term's: the softened one (eps2 == 0: ds2 == d2, d2 is never -0) */
    const double ds = (double)sqrtf(ds2);
    const float s = (float)(g * (double)nd->total_mass / ((ds * ds) * ds));
    acc[0] = acc[0] + s * (nd->com[0] - pi[0]);
    acc[1] = acc[1] + s * (nd->com[1] - pi[1]);
    acc[2] = acc[2] + s * (nd->com[2] - pi[2]);
  } else if (!leaf) {
    for (int i = 0; i < 8; ++i) forces(t, nd->child[i], pi, theta, g, eps2, acc);
  }
}

/* CreateOctree (OctreeSearch.cpp:74-89) of the n bodies, then the walk from each of the m points.  acc: m x 3.
 * Returns 0, 1 past depth 200, 2 out of memory. */
API int bhp_field_f32(int n, const float *pos, const float *mass, const float root_origin[3], float root_size, float theta, double g,
                      float eps2, int div_mode, int m, const float *pts, float *acc, float root_com_out[3], int *node_count_out) {
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
    forces(&t, root, &pts[3 * k], theta, g, eps2, a);
    acc[3 * k + 0] = a[0]; acc[3 * k + 1] = a[1]; acc[3 * k + 2] = a[2];
  }
  if (root_com_out) memcpy(root_com_out, t.nodes[root].com, sizeof(float) * 3);
  if (node_count_out) *node_count_out = t.count;
  free(t.nodes);
  return 0;
}
