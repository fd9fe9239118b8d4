// oracle/ref_driver.cpp — one program around an AOctreeSearch, built twice (TEST INFRASTRUCTURE ONLY):
//
//   oracle/_ref/nbody_ref   this file + the REFERENCE's own Source/NBody/OctreeSearch.cpp, unchanged, against the stand-in headers
//                           of oracle/ue4_standin/ (oracle/Makefile).  What it prints is what the reference computes.
//   the adapter program     this file + integration/ue4/OctreeSearch.cpp + libnbody_amd, with -DNBODY_DRIVER_ADAPTER
//                           (tests/test_reference_parity_gpu.py builds it at test time).  Needs a GPU.
//
// Usage: ref_driver SCENE RESULT.  Both files are little-endian binary; oracle/reference.py writes the one and reads the other.
//   SCENE   "NBSCENE1", int32 n, n FParticle records of 40 bytes, then text: one command per line
//   RESULT  "NBRESLT1", then one block per command, in order
// Commands:
//   ticks DT FRAMES SHOW_OCTREE    spawn the actor, BeginPlay, load the scene, set PhDeltaTime and ShowOctree, Tick FRAMES times — what
//                                  the Blueprints do.  Per frame: n records; float Size; float[3] the root's centre of mass (NaN from the
//                                  adapter: its tree is on the device); int32 calls; per draw call, in the order made since the frame's
//                                  FlushPersistentDebugLines, int32 kind (0 = DrawDebugBox, 1 = DrawDebugPoint) and float[6]
//                                  (box: Center, Extent; point: Position, Size, 0, 0).
//   forces THETA OX OY OZ SIZE     (reference build only) the reference's Octree class directly: Octree(Origin, SIZE), Add every body,
//                                  ComputeMass, ComputeForces(p, THETA) per body.  float[n][3] accelerations; float[3] root centre of mass.
// Floats in commands are read by strtof (hexadecimal floats keep every bit).  Exit status 0 = every command ran.
// The reference does not terminate on coincident bodies (Octree::Add recurses for ever): callers run this program as a child under
// a time limit and send no such scene; the program also ends itself after 60 s.
#include "NBody.h"
#include "OctreeSearch.h"

#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

// what Engine.h declares and the engine would define
const FVector FVector::ZeroVector(0.f, 0.f, 0.f);
const FColor FColor::Red(255, 0, 0), FColor::Black(0, 0, 0);

static_assert(sizeof(FParticle) == 40, "FParticle is the 40-byte record: Mass, Position, Velocity, Acceleration");

// ---- the recording renderer ----
struct DrawCall { int32 Kind; float V[6]; };
static std::vector<DrawCall> GCalls;

void FlushPersistentDebugLines(const UWorld *) { GCalls.clear(); }
void DrawDebugBox(const UWorld *, FVector const &Center, FVector const &Extent, FColor const &, bool, float, uint8) {
  const DrawCall C = {0, {Center.X, Center.Y, Center.Z, Extent.X, Extent.Y, Extent.Z}};
  GCalls.push_back(C);
}
void DrawDebugPoint(const UWorld *, FVector const &Position, float Size, FColor const &, bool, float, uint8) {
  const DrawCall C = {1, {Position.X, Position.Y, Position.Z, Size, 0.f, 0.f}};
  GCalls.push_back(C);
}

// ---- the one place where the two builds differ: what only one of the two AOctreeSearch classes can do ----
#ifdef NBODY_DRIVER_ADAPTER
// A host-made scene by the documented route: the actor is initialised the way BP_NBodyHUD does it, the host
// announces that it is about to refill the array, refills it, and pushes the records.
static bool LoadScene(AOctreeSearch &A, const std::vector<FParticle> &Scene) {
  A.CreateSpacePoints((int32)Scene.size(), 200.f);
  if (!A.Initialized) return false;                             // (no HIP device, or the context could not be created)
  A.ReleaseStorage();
  A.Particles.Empty();
  A.Particles.SetNumUninitialized((int32)Scene.size());
  memcpy(A.Particles.GetData(), Scene.data(), Scene.size() * sizeof(FParticle));
  A.PushParticles();
  return A.Initialized && A.Particles.Num() == (int32)Scene.size();
}
static FVector RootCentreOfMass(const AOctreeSearch &) {        // class Octree is opaque in the adapter: the tree is on the device
  const float NaN = std::numeric_limits<float>::quiet_NaN();
  return FVector(NaN, NaN, NaN);
}
static bool Forces(std::vector<FParticle> &, float, const FVector &, float, FVector &) { return false; }
#else
// The reference has no way in but CreateSpacePoints and its unseeded generator: fill the array and set the flag it sets (.cpp:71).
static bool LoadScene(AOctreeSearch &A, const std::vector<FParticle> &Scene) {
  A.Particles.SetNum((int32)Scene.size());
  for (size_t i = 0; i < Scene.size(); ++i) A.Particles[(int32)i] = Scene[i];
  A.Initialized = true;
  return true;
}
static FVector RootCentreOfMass(const AOctreeSearch &A) { return A.ParticleOctree->GetCenterOfMass(); }
// CreateOctree's body (OctreeSearch.cpp:79-86) with the root and the opening angle as arguments
static bool Forces(std::vector<FParticle> &P, float Theta, const FVector &Origin, float Size, FVector &CentreOfMass) {
  Octree *Tree = new Octree(Origin, Size);
  for (size_t i = 0; i < P.size(); ++i) Tree->Add(&P[i]);
  Tree->ComputeMass();
  for (size_t i = 0; i < P.size(); ++i) {
    P[i].Acceleration = FVector::ZeroVector;
    Tree->ComputeForces(&P[i], Theta);
  }
  CentreOfMass = Tree->GetCenterOfMass();
  delete Tree;
  return true;
}
#endif

static void Put(FILE *F, const void *P, size_t Bytes) {
  if (Bytes && fwrite(P, 1, Bytes, F) != Bytes) { fprintf(stderr, "ref_driver: write failed\n"); exit(3); }
}
static void PutVector(FILE *F, const FVector &V) { const float X[3] = {V.X, V.Y, V.Z}; Put(F, X, sizeof X); }

static int Ticks(FILE *Out, const std::vector<FParticle> &Scene, float Dt, int Frames, bool ShowOctree) {
  AOctreeSearch *A = new AOctreeSearch();                       // BP_NBodyHUD: SpawnActor ...
  A->BeginPlay();
  if (!LoadScene(*A, Scene)) { fprintf(stderr, "ref_driver: the actor did not take the scene (no device?)\n"); delete A; return 2; }
  A->PhDeltaTime = Dt;                                          // BP_ScreenUI writes both
  A->ShowOctree = ShowOctree;
  for (int Frame = 0; Frame < Frames; ++Frame) {
    A->Tick(1.f / 60);                                          // (DeltaSeconds is ignored: OctreeSearch.cpp:21-34)
    if (A->Particles.Num() != (int32)Scene.size()) { fprintf(stderr, "ref_driver: frame %d lost the records\n", Frame); delete A; return 2; }
    Put(Out, A->Particles.GetData(), Scene.size() * sizeof(FParticle));
    Put(Out, &A->Size, sizeof(float));
    PutVector(Out, RootCentreOfMass(*A));
    const int32 Calls = (int32)GCalls.size();
    Put(Out, &Calls, sizeof Calls);
    Put(Out, GCalls.data(), GCalls.size() * sizeof(DrawCall));
  }
  A->CleanParticles();
  delete A;
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s SCENE RESULT\n", argv[0]); return 64; }
  alarm(60);
  FILE *In = fopen(argv[1], "rb");
  if (!In) { perror(argv[1]); return 66; }
  char Magic[8];
  int32 N = 0;
  if (fread(Magic, 1, 8, In) != 8 || memcmp(Magic, "NBSCENE1", 8) || fread(&N, 4, 1, In) != 1 || N < 1) {
    fprintf(stderr, "ref_driver: %s is no scene file\n", argv[1]);
    return 65;
  }
  std::vector<FParticle> Scene((size_t)N);
  if (fread(Scene.data(), sizeof(FParticle), (size_t)N, In) != (size_t)N) { fprintf(stderr, "ref_driver: short scene\n"); return 65; }
  FILE *Out = fopen(argv[2], "wb");
  if (!Out) { perror(argv[2]); return 73; }
  Put(Out, "NBRESLT1", 8);

  char Line[512];
  while (fgets(Line, sizeof Line, In)) {
    char *Save = NULL;
    const char *Word = strtok_r(Line, " \t\r\n", &Save);
    if (!Word) continue;
    std::vector<const char *> Args;
    for (const char *T; (T = strtok_r(NULL, " \t\r\n", &Save));) Args.push_back(T);
    if (!strcmp(Word, "ticks") && Args.size() == 3) {
      const int Status = Ticks(Out, Scene, strtof(Args[0], NULL), atoi(Args[1]), atoi(Args[2]) != 0);
      if (Status) return Status;
    } else if (!strcmp(Word, "forces") && Args.size() == 5) {
      std::vector<FParticle> P(Scene);
      FVector CentreOfMass(0.f, 0.f, 0.f);
      const FVector Origin(strtof(Args[1], NULL), strtof(Args[2], NULL), strtof(Args[3], NULL));
      if (!Forces(P, strtof(Args[0], NULL), Origin, strtof(Args[4], NULL), CentreOfMass)) {
        fprintf(stderr, "ref_driver: `forces` needs the reference's Octree class: the reference build only\n");
        return 64;
      }
      for (size_t i = 0; i < P.size(); ++i) PutVector(Out, P[i].Acceleration);
      PutVector(Out, CentreOfMass);
    } else {
      fprintf(stderr, "ref_driver: bad command `%s`\n", Word);
      return 64;
    }
  }
  fclose(In);
  if (fclose(Out)) { perror(argv[2]); return 74; }
  return 0;
}
