// Test-only driver of the transmission table's sigma rows (loupiote_amd/csrc/material_tables.h, SPEC.md §28; tests/test_volume.py): builds a scene through the C ABI
// from the commands on stdin, derives the material side tables and prints the transmission table as one JSON line per run.  Whitespace-separated tokens:
//   scene MATERIALS                 a fresh scene with that many (default) materials, no instance, no layout
//   trans M FACTOR IOR THIN         lpt_scene_set_material_transmission
//   atten M R G B DISTANCE          lpt_scene_set_material_attenuation (DISTANCE may be inf)
//   inst MATERIAL FIRST COUNT       an instance and its run of baked triangles
//   tris N                          the baked triangle count
//   derive                          run and print: the records, the sigma rows (`more`) and the per-triangle entries
// Records and rows are printed as the bit patterns of their four floats.
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
        } else if (cmd == "trans") {
            float factor, ior;
            in >> a >> factor >> ior >> b;
            if (lpt_scene_set_material_transmission(&scene, (uint32_t)a, factor, ior, (uint32_t)b) != LPT_OK) { std::fprintf(stderr, "trans: %s\n", lpt_last_error()); return 2; }
        } else if (cmd == "atten") {
            std::string tok[4];
            in >> a >> tok[0] >> tok[1] >> tok[2] >> tok[3];
            const float color[3] = {std::strtof(tok[0].c_str(), nullptr), std::strtof(tok[1].c_str(), nullptr), std::strtof(tok[2].c_str(), nullptr)};
            if (lpt_scene_set_material_attenuation(&scene, (uint32_t)a, color, std::strtof(tok[3].c_str(), nullptr)) != LPT_OK) { std::fprintf(stderr, "atten: %s\n", lpt_last_error()); return 2; }
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
            std::printf("{\"status\": %d, ", st);
            print_recs("recs", t[MAT_TRANS].recs);
            std::printf(", ");
            print_recs("more", t[MAT_TRANS].more);
            std::printf(", \"tri\": [");
            for (size_t i = 0; i < t[MAT_TRANS].tri.size(); ++i) std::printf("%s%u", i ? ", " : "", t[MAT_TRANS].tri[i]);
            std::printf("], \"others\": %zu}\n", t[MAT_ALPHA].more.size() + t[MAT_EMIS].more.size() + t[MAT_NMAP].more.size());
        } else {
            std::fprintf(stderr, "unknown command: %s\n", cmd.c_str());
            return 2;
        }
        if (in.fail() && !in.eof()) { std::fprintf(stderr, "bad arguments: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
