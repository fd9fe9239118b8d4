/*
 * bh_pot_ref.c — the reference's octree walked from arbitrary points, returning the POTENTIAL next to the acceleration.  TEST
 * INFRASTRUCTURE ONLY (tests/bh_pot_ref.py builds and loads it; nothing under parallelnbody_amd/ links it): the yardstick of
 * nbody_potential_at, nbody_get_potentials and nbody_energy_fast at theta > 0.
 *
 * The tree build and the acceleration are those of tests/cpp/bh_probe_ref.c, restated line for line (tests/test_bh_pot_ref.py pins
 * them to it in every byte).  The potential is build-defined (the reference computes none): in the same walk an accepted node adds,
 * in double,
 *         g * (double)M / (double)ds,        ds = sqrtf(d2 + eps2)   (the softened distance the force term uses)
 * to a double sum in walk order; the result is phi64 = -sum and phi = (float)phi64.
 *
 * The tree is the one of tests/cpp/bh_softened_ref.c, restated:
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

#define API __attribute__((visibility("default")))
#define MAX_DEPTH 200

typedef struct {
  int particle;
  float origin[3];
  float size;
  float total_mass;
  float com[3];
  int child[8];
} onode;

typedef struct {
  onode *nodes;
  int count, cap;
  const float *pos, *mass;
  int overflow;
  int div_mode;
} otree;

static int node_new(otree *t, const float origin[3], float size) {
  if (t->count == t->cap) {
    int ncap = t->cap ? t->cap * 2 : 1024;
    onode *nn = (onode *)realloc(t->nodes, (size_t)ncap * sizeof(onode));
    if (!nn) { t->overflow = 2; return -1; }
    t->nodes = nn; t->cap = ncap;
  }
  onode *nd = &t->nodes[t->count];
  nd->particle = -1;
  memcpy(nd->origin, origin, sizeof(float) * 3);
  nd->size = size;
  nd->total_mass = 0.0f;
  nd->com[0] = nd->com[1] = nd->com[2] = 0.0f;
  for (int i = 0; i < 8; ++i) nd->child[i] = -1;
  return t->count++;
}

static int is_leaf(const otree *t, int k) { return t->nodes[k].child[0] == -1; }

static int octant(const otree *t, int k, const float p[3]) {
  const onode *nd = &t->nodes[k];
  return (p[0] >= nd->origin[0] ? 4 : 0) | (p[1] >= nd->origin[1] ? 2 : 0) | (p[2] >= nd->origin[2] ? 1 : 0);
}

static void add(otree *t, int k, int particle, int depth) {
  if (t->overflow) return;
  if (depth > MAX_DEPTH) { t->overflow = 1; return; }
  if (is_leaf(t, k)) {
    if (t->nodes[k].particle == -1) {
      t->nodes[k].particle = particle;
      return;
    }
    const int old = t->nodes[k].particle;
    t->nodes[k].particle = -1;
    for (int i = 0; i < 8; ++i) {
      float c[3];
      const float sz = t->nodes[k].size;
      memcpy(c, t->nodes[k].origin, sizeof(c));
      c[0] = (float)((double)c[0] + (double)sz * ((i & 4) ? 0.5 : -0.5));
      c[1] = (float)((double)c[1] + (double)sz * ((i & 2) ? 0.5 : -0.5));
      c[2] = (float)((double)c[2] + (double)sz * ((i & 1) ? 0.5 : -0.5));
      const int ch = node_new(t, c, (float)(0.5 * (double)sz));
      if (ch < 0) return;
      t->nodes[k].child[i] = ch;
    }
    add(t, t->nodes[k].child[octant(t, k, &t->pos[3 * old])], old, depth + 1);
    add(t, t->nodes[k].child[octant(t, k, &t->pos[3 * particle])], particle, depth + 1);
  } else {
    add(t, t->nodes[k].child[octant(t, k, &t->pos[3 * particle])], particle, depth + 1);
  }
}

static void compute_mass(otree *t, int k) {
  if (is_leaf(t, k)) {
    const int p = t->nodes[k].particle;
    if (p != -1) {
      memcpy(t->nodes[k].com, &t->pos[3 * p], sizeof(float) * 3);
      t->nodes[k].total_mass = t->mass[p];
    }
    return;
  }
  for (int i = 0; i < 8; ++i) {
    const int c = t->nodes[k].child[i];
    compute_mass(t, c);
    onode *nd = &t->nodes[k];
    const onode *ch = &t->nodes[c];
    nd->total_mass = nd->total_mass + ch->total_mass;
    nd->com[0] = nd->com[0] + ch->total_mass * ch->com[0];
    nd->com[1] = nd->com[1] + ch->total_mass * ch->com[1];
    nd->com[2] = nd->com[2] + ch->total_mass * ch->com[2];
  }
  onode *nd = &t->nodes[k];
  if (nd->total_mass != 0.0f) {
    if (t->div_mode == 0) {
      const float rv = 1.0f / nd->total_mass;
      nd->com[0] *= rv; nd->com[1] *= rv; nd->com[2] *= rv;
    } else {
      nd->com[0] = nd->com[0] / nd->total_mass; nd->com[1] = nd->com[1] / nd->total_mass; nd->com[2] = nd->com[2] / nd->total_mass;
    }
  } else {
    memcpy(nd->com, nd->origin, sizeof(float) * 3);
  }
}

static void forces(const otree *t, int k, const float pi[3], float theta, double g, float eps2, float acc[3], double *psum) {
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
    *psum = *psum + g * (double)nd->total_mass / ds;       /* the potential's term: one correctly rounded double division */
  } else if (!leaf) {
    for (int i = 0; i < 8; ++i) forces(t, nd->child[i], pi, theta, g, eps2, acc, psum);
  }
}

/* CreateOctree (OctreeSearch.cpp:74-89) of the n bodies, then the walk from each of the m points.  acc: m x 3; phi64, phi: m each.
 * root_mass_out: the root's TotalMass.  Returns 0, 1 past depth 200, 2 out of memory. */
API int bhpot_walk_f32(int n, const float *pos, const float *mass, const float root_origin[3], float root_size, float theta, double g,
                       float eps2, int div_mode, int m, const float *pts, float *acc, double *phi64, float *phi, float root_com_out[3],
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
    double sum = 0.0;
    forces(&t, root, &pts[3 * k], theta, g, eps2, a, &sum);
    acc[3 * k + 0] = a[0]; acc[3 * k + 1] = a[1]; acc[3 * k + 2] = a[2];
    phi64[k] = -sum;
    phi[k] = (float)phi64[k];
  }
  if (root_com_out) memcpy(root_com_out, t.nodes[root].com, sizeof(float) * 3);
  if (root_mass_out) *root_mass_out = t.nodes[root].total_mass;
  if (node_count_out) *node_count_out = t.count;
  free(t.nodes);
  return 0;
}
