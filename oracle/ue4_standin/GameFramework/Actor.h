// oracle/ue4_standin/GameFramework/Actor.h — the AActor surface AOctreeSearch uses (see Engine.h next to this directory): virtual
// BeginPlay / Tick for `override` and Super::, GetWorld() (there is no world: NULL), GetActorLocation() (the origin, where
// BP_NBodyHUD spawns the actor), PrimaryActorTick.bCanEverTick.
#pragma once
#include "Engine.h"

class UWorld;

struct FActorTickFunction {
  bool bCanEverTick;
  FActorTickFunction() : bCanEverTick(false) {}
};

class AActor {
 public:
  AActor() {}
  virtual ~AActor() {}
  virtual void BeginPlay() {}
  virtual void Tick(float /*DeltaSeconds*/) {}
  UWorld *GetWorld() const { return NULL; }
  FVector GetActorLocation() const { return FVector(0.f, 0.f, 0.f); }
  FActorTickFunction PrimaryActorTick;
};
