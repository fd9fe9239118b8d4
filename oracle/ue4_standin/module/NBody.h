// oracle/ue4_standin/module/NBody.h — the module's precompiled header by name, for the ADAPTER build only
// (integration/ue4/OctreeSearch.cpp includes "NBody.h").  The reference build never sees this file: its `#include "NBody.h"` finds
// Source/NBody/NBody.h next to its own sources, and that one includes "Engine.h" just as this one does.
#pragma once
#include "Engine.h"
