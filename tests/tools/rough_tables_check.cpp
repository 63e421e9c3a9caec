// Test-only driver of the transmission table's rough bit (loupiote_amd/csrc/material_tables.h, SPEC.md §29; tests/test_rough_transmission.py): builds a scene through the
// C ABI from the commands on stdin, derives the material side tables and prints the transmission table as one JSON line per run.  Whitespace-separated tokens:
//   scene MATERIALS                 a fresh scene with that many (default) materials, no instance, no layout
//   trans M FACTOR IOR THIN         lpt_scene_set_material_transmission
//   rough M ON                      lpt_scene_set_material_transmission_rough; a rejected call prints its status and changes nothing
//   atten M R G B DISTANCE          lpt_scene_set_material_attenuation
//   inst MATERIAL FIRST COUNT       an instance and its run of baked triangles
//   tris N                          the baked triangle count
//   derive                          run and print: the records and rows as the bit patterns of their four floats, the per-triangle entries, and what the two
//                                   device-side readers make of every record's third float: thin (z != 0) and rough (the sign bit)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../loupiote_amd/csrc/material_tables.h"

using namespace lpt;

static void print_recs(const char *name, const std::vector<MaterialRec> &v) {
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) {
        uint32_t u[4];
        std::memcpy(u, &v[i], 16);
        std::printf("%s[%u, %u, %u, %u]", i ? ", " : "", u[0], u[1], u[2], u[3]);
    }
    std::printf("]");
}

int main() {
    lpt_scene scene;
    std::vector<uint32_t> inst_first, inst_count;
    uint32_t n_tris = 0;
    int rejected = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        long long a = 0, b = 0, c = 0;
        if (cmd == "scene") {
            in >> a;
            scene = lpt_scene();
            scene.materials.resize((size_t)a);
            for (lpt_material &m : scene.materials) { m = lpt_material{}; m.albedo_texture = m.mra_texture = LPT_INVALID_INDEX; m.color[3] = 1.0f; }
            inst_first.clear(); inst_count.clear();
            n_tris = 0;
            rejected = 0;
        } else if (cmd == "trans") {
            float factor, ior;
            in >> a >> factor >> ior >> b;
            if (lpt_scene_set_material_transmission(&scene, (uint32_t)a, factor, ior, (uint32_t)b) != LPT_OK) { std::fprintf(stderr, "trans: %s\n", lpt_last_error()); return 2; }
        } else if (cmd == "rough") {
            in >> a >> b;
            if (lpt_scene_set_material_transmission_rough(&scene, (uint32_t)a, (uint32_t)b) != LPT_OK) ++rejected;
        } else if (cmd == "atten") {
            float col[3], dist;
            in >> a >> col[0] >> col[1] >> col[2] >> dist;
            if (lpt_scene_set_material_attenuation(&scene, (uint32_t)a, col, dist) != LPT_OK) { std::fprintf(stderr, "atten: %s\n", lpt_last_error()); return 2; }
        } else if (cmd == "inst") {
            in >> a >> b >> c;
            lpt_instance inst{};
            inst.material_index = (uint32_t)a;
            scene.instances.push_back(inst);
            inst_first.push_back((uint32_t)b); inst_count.push_back((uint32_t)c);
        } else if (cmd == "tris") {
            in >> a;
            n_tris = (uint32_t)a;
        } else if (cmd == "derive") {
            MaterialTable t[MAT_KINDS];
            const int st = derive_material_tables(scene, inst_first, inst_count, n_tris, std::vector<uint8_t>(), t);
            std::printf("{\"status\": %d, \"rejected\": %d, ", st, rejected);
            print_recs("recs", t[MAT_TRANS].recs);
            std::printf(", ");
            print_recs("more", t[MAT_TRANS].more);
            std::printf(", \"tri\": [");
            for (size_t i = 0; i < t[MAT_TRANS].tri.size(); ++i) std::printf("%s%u", i ? ", " : "", t[MAT_TRANS].tri[i]);
            std::printf("], \"thin\": [");
            for (size_t i = 0; i < t[MAT_TRANS].recs.size(); ++i) std::printf("%s%d", i ? ", " : "", t[MAT_TRANS].recs[i].z != 0.0f ? 1 : 0);
            std::printf("], \"rough\": [");
            for (size_t i = 0; i < t[MAT_TRANS].recs.size(); ++i) {
                uint32_t u;
                std::memcpy(&u, &t[MAT_TRANS].recs[i].z, 4);
                std::printf("%s%u", i ? ", " : "", u >> 31);
            }
            std::printf("]}\n");
        } else {
            std::fprintf(stderr, "unknown command: %s\n", cmd.c_str());
            return 2;
        }
        if (in.fail() && !in.eof()) { std::fprintf(stderr, "bad arguments: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
