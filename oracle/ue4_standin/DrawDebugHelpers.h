// oracle/ue4_standin/DrawDebugHelpers.h — the three debug-draw calls of OctreeSearch.cpp:24, 40, 41 with their 4.9 signatures.
// Declared here, DEFINED by the program that links the actor (oracle/ref_driver.cpp records every call in order).
#pragma once
#include "Engine.h"

void FlushPersistentDebugLines(const UWorld *InWorld);
void DrawDebugBox(const UWorld *InWorld, FVector const &Center, FVector const &Extent, FColor const &Color, bool bPersistentLines = false,
                  float LifeTime = -1.f, uint8 DepthPriority = 0);
void DrawDebugPoint(const UWorld *InWorld, FVector const &Position, float Size, FColor const &PointColor, bool bPersistentLines = false,
                    float LifeTime = -1.f, uint8 DepthPriority = 0);
