// the header layer of the instance worlds compiles and links (tests/test_world_query_cpu.py); never run against a device
#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"
int main(int argc, char**) { if (argc > 99) { psm::InstanceWorld w(4); psm::TriangleHierarchy* t = nullptr; w.add(t); w.commit(); w.setTransform(0, glm::mat4(1.0f)); w.refresh(); return (int)w.count(); } return 0; }
