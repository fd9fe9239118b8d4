// oracle/ue4_standin/OctreeSearch.generated.h — UnrealHeaderTool would generate this file from OctreeSearch.h.  Of all it generates
// the sources use one thing: the base class under the name Super inside AOctreeSearch (`Super::BeginPlay()`, OctreeSearch.cpp:17, 23).
// GENERATED_BODY leaves the access level private, as UnrealHeaderTool's does; both headers follow it with `public:`.
#pragma once
#undef GENERATED_BODY
#define GENERATED_BODY(...) public: typedef AActor Super; private:
