// oracle/ue4_standin/Engine.h — a functional stand-in for the part of Unreal Engine 4.9 that Milias/ParallelNbody's module NBody
// uses, so that the reference's own OctreeSearch.{h,cpp} compile UNCHANGED with a plain g++ (oracle/Makefile, target _ref/nbody_ref)
// and so that this repository's drop-in, integration/ue4/OctreeSearch.{h,cpp}, links and runs against libnbody_amd
// (tests/test_reference_parity_gpu.py).  Every line here is this project's own text, written from the 4.9 API as documented; none of
// it is engine code.  What it pins and what it does not: DESIGN.md §2.
//
// The rule that makes the build worth having: FVector has exactly the overloads the engine has — every scalar is `float`, there is
// no double overload anywhere — so the COMPILER applies the reference's conversions (`Size * (i & 4 ? 0.5 : -0.5)` is a double
// product added to a float and rounded once; `1e4*TotalMass/pow(d,3) * FVector` is a double narrowed to the float Scale of
// operator*(float, FVector)); nobody restates them by reading.
// Compile with -ffp-contract=off and without -ffast-math: the engine's operators are separate fp32 multiplies and adds.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

typedef int32_t int32;
typedef uint8_t uint8;

// UnrealHeaderTool's markers: nothing for a plain compiler.  (GENERATED_BODY: OctreeSearch.generated.h.)
#define USTRUCT(...)
#define UCLASS(...)
#define UPROPERTY(...)
#define UFUNCTION(...)
#define GENERATED_USTRUCT_BODY(...)
#define NBODY_API   // UnrealBuildTool's export macro of the module NBody

// Engine/Source/Runtime/Core/Public/Math/Vector.h (4.9): three floats, component-wise operators, each one fp32 operation per component.
struct FVector {
  float X, Y, Z;

  FVector() {}                                                     // FORCEINLINE FVector(): leaves the components uninitialised
  FVector(float InX, float InY, float InZ) : X(InX), Y(InY), Z(InZ) {}
  static const FVector ZeroVector;                                 // (0, 0, 0); defined by the program (oracle/ref_driver.cpp)

  // operator+(const FVector& V) const: FVector(X + V.X, Y + V.Y, Z + V.Z)
  FVector operator+(const FVector &V) const { return FVector(X + V.X, Y + V.Y, Z + V.Z); }
  // operator-(const FVector& V) const: FVector(X - V.X, Y - V.Y, Z - V.Z)
  FVector operator-(const FVector &V) const { return FVector(X - V.X, Y - V.Y, Z - V.Z); }
  // operator*(float Scale) const: FVector(X * Scale, Y * Scale, Z * Scale)
  FVector operator*(float Scale) const { return FVector(X * Scale, Y * Scale, Z * Scale); }
  // operator+=(const FVector& V): X += V.X; Y += V.Y; Z += V.Z
  FVector operator+=(const FVector &V) { X += V.X; Y += V.Y; Z += V.Z; return *this; }
  // operator/=(float V): const float RV = 1.f/V; X *= RV; Y *= RV; Z *= RV — a reciprocal multiply, not three divisions
  FVector operator/=(float V) { const float RV = 1.f / V; X *= RV; Y *= RV; Z *= RV; return *this; }
  // GetAbsMax(): FMath::Max(FMath::Max(FMath::Abs(X), FMath::Abs(Y)), FMath::Abs(Z)), with Max(A, B) = (A >= B) ? A : B
  float GetAbsMax() const {
    const float AX = fabsf(X), AY = fabsf(Y), AZ = fabsf(Z);
    const float M = (AX >= AY) ? AX : AY;
    return (M >= AZ) ? M : AZ;
  }
  // Dist(V1, V2): FMath::Sqrt(FMath::Square(V2.X-V1.X) + FMath::Square(V2.Y-V1.Y) + FMath::Square(V2.Z-V1.Z)); Sqrt is sqrtf, the sum
  // runs left to right in fp32
  static float Dist(const FVector &V1, const FVector &V2) {
    const float DX = V2.X - V1.X, DY = V2.Y - V1.Y, DZ = V2.Z - V1.Z;
    return sqrtf(DX * DX + DY * DY + DZ * DZ);
  }
};
// the non-member operator*(float Scale, const FVector& V): V.operator*(Scale)
inline FVector operator*(float Scale, const FVector &V) { return V.operator*(Scale); }

// Math/Color.h: only named, never computed with
struct FColor {
  uint8 B, G, R, A;
  FColor() {}
  FColor(uint8 InR, uint8 InG, uint8 InB, uint8 InA = 255) : B(InB), G(InG), R(InR), A(InA) {}
  static const FColor Red, Black;
};

// Math/Box.h, Math/UnrealMathUtility.h: what CreateSpacePoints names (OctreeSearch.cpp:58-72).  No test calls CreateSpacePoints of the
// reference build — the engine's generator is global and unseeded, there is nothing to compare — so these only have to compile:
// the box's Min corner, the range's lower end, the unit X vector.
struct FBox {
  FVector Min, Max;
  FBox(const FVector &InMin, const FVector &InMax) : Min(InMin), Max(InMax) {}
};
struct FMath {
  static FVector RandPointInBox(const FBox &Box) { return Box.Min; }
  static float RandRange(float InMin, float) { return InMin; }
  static FVector VRand() { return FVector(1.f, 0.f, 0.f); }
};

// Containers/Array.h over std::vector: the members the reference and the adapter call
template <typename T> class TArray {
  std::vector<T> Data;

 public:
  int32 Num() const { return (int32)Data.size(); }
  T *GetData() { return Data.data(); }
  const T *GetData() const { return Data.data(); }
  void SetNum(int32 NewNum) { Data.resize((size_t)NewNum); }
  void SetNumUninitialized(int32 NewNum) { Data.resize((size_t)NewNum); }   // (initialised here: harmless)
  void Empty() { Data.clear(); }
  T &operator[](int32 Index) { return Data[(size_t)Index]; }
  const T &operator[](int32 Index) const { return Data[(size_t)Index]; }
};

#include "GameFramework/Actor.h"
#include "DrawDebugHelpers.h"   // Engine.h brings the debug-draw calls in 4.9: the reference includes nothing else for them
