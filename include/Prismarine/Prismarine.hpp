#pragma once
// Prismarine/Prismarine.hpp -- umbrella include (reference Include/Prismarine/Prismarine.hpp:3-9)
#include "Utils.hpp"
#include "Structs.hpp"
#include "Radix.hpp"
#include "VertexInstance.hpp"
#include "TextureSet.hpp"
#include "MaterialSet.hpp"
#include "TriangleHierarchy.hpp"
#include "QueryScene.hpp"          // addition: the queries over several hierarchies at once (psm_scene_*_dev)
#include "InstancedScene.hpp"      // addition: the same over instances, a hierarchy and a rigid pose each (psm_instances_*_dev)
#include "InstanceWorld.hpp"       // addition: the same without the limit of 32, under a top-level tree on the device (psm_world_*)
#include "Pipeline.hpp"
#include "FrameBatch.hpp"   // addition: several frames in flight (psm_lanes_render)
