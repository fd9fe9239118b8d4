/*
 * bh_ref_tree.h — the octree the CPU yardsticks of the theta > 0 path share (bh_softened_ref.c, bh_probe_ref.c, bh_pot_ref.c).  TEST
 * INFRASTRUCTURE ONLY.  A copy of the tree of oracle/nbody_oracle.c, which stays as it is:
 *   - Octree::Add (OctreeSearch.h:60-81) with the children's centres in double rounded to fp32, cut off past depth 200;
 *   - ComputeMass (.h:83-97) under both readings of `/=` (div_mode 0: the fp32 reciprocal multiplied, 1: three divisions).
 * The walks (ComputeForces, .h:99-108) are the including files' own: they differ in what they return.
 * Compile with -ffp-contract=off and without -ffast-math, as the oracle.
 */
#ifndef BH_REF_TREE_H
#define BH_REF_TREE_H

#include <stdlib.h>
#include <string.h>

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

#endif
