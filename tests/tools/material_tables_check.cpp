// Test-only driver of loupiote_amd/csrc/material_tables.h (tests/test_material_tables.py): builds a scene from the commands on stdin, runs the derivation of the
// four material side tables or the residency of the plain images, and prints one JSON line per run.  Whitespace-separated tokens; -1 stands for LPT_INVALID_INDEX:
//   scene IMAGES MATERIALS          a fresh scene with that many (empty) images and (default) materials, no instance, no layout
//   mat M ALBEDO MRA COLOR_W PAIRED the material's two textures, its color.w, and whether the two textures were stored as a pair
//   alpha M MODE CUTOFF IMAGE | trans M FACTOR IOR THIN | emis M R G B IMAGE | nmap M IMAGE SCALE      a side-table entry (the tables grow to hold it)
//   inst MATERIAL FIRST COUNT       an instance and its run of baked triangles;  inst MATERIAL  alone: an instance beyond the baked layout
//   tris N | resident B B ...       the baked triangle count; one flag per image (ends at the end of the line)
//   derive | residency              run and print
// Records are printed as the bit patterns of their four floats.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../loupiote_amd/csrc/material_tables.h"

using namespace lpt;

static uint32_t index_of(long long v) { return v < 0 ? LPT_INVALID_INDEX : (uint32_t)v; }
template <typename T>
static T &slot(std::vector<T> &v, size_t i) {
    if (v.size() <= i) v.resize(i + 1);
    return v[i];
}

int main() {
    lpt_scene scene;
    std::vector<uint32_t> inst_first, inst_count;
    std::vector<uint8_t> resident, paired;
    uint32_t n_tris = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        long long a = 0, b = 0, c = 0;
        if (cmd == "scene") {
            in >> a >> b;
            scene = lpt_scene();
            scene.images.resize((size_t)a);
            scene.materials.resize((size_t)b);
            for (lpt_material &m : scene.materials) { m = lpt_material{}; m.albedo_texture = m.mra_texture = LPT_INVALID_INDEX; m.color[3] = 1.0f; }
            paired.assign((size_t)b, 0);
            inst_first.clear(); inst_count.clear(); resident.clear();
            n_tris = 0;
        } else if (cmd == "mat") {
            float w;
            long long p;
            in >> a >> b >> c >> w >> p;
            lpt_material &m = scene.materials.at((size_t)a);
            m.albedo_texture = index_of(b); m.mra_texture = index_of(c); m.color[3] = w;
            paired.at((size_t)a) = (uint8_t)p;
        } else if (cmd == "alpha") {
            MaterialAlpha v;
            in >> a >> v.mode >> v.cutoff >> b;
            v.image = index_of(b);
            slot(scene.alpha, (size_t)a) = v;
        } else if (cmd == "trans") {
            MaterialTransmission v;
            in >> a >> v.factor >> v.ior >> v.thin_walled;
            slot(scene.transmission, (size_t)a) = v;
        } else if (cmd == "emis") {
            MaterialEmission v;
            in >> a >> v.le[0] >> v.le[1] >> v.le[2] >> b;
            v.image = index_of(b);
            slot(scene.emission, (size_t)a) = v;
        } else if (cmd == "nmap") {
            MaterialNormalMap v;
            in >> a >> b >> v.scale;
            v.image = index_of(b);
            slot(scene.normal_map, (size_t)a) = v;
        } else if (cmd == "inst") {
            in >> a;
            lpt_instance inst{};
            inst.material_index = index_of(a);
            scene.instances.push_back(inst);
            if (in >> b >> c) { inst_first.push_back((uint32_t)b); inst_count.push_back((uint32_t)c); }
        } else if (cmd == "tris") {
            in >> a;
            n_tris = (uint32_t)a;
        } else if (cmd == "resident") {
            resident.clear();
            while (in >> a) resident.push_back((uint8_t)a);
        } else if (cmd == "derive") {
            MaterialTable t[MAT_KINDS];
            const int st = derive_material_tables(scene, inst_first, inst_count, n_tris, resident, t);
            std::printf("{\"status\": %d, \"error\": \"%s\", \"tables\": [", st, st == LPT_OK ? "" : lpt_last_error());
            for (int k = 0; k < MAT_KINDS; ++k) {
                std::printf("%s{\"section\": %d, \"recs\": [", k ? ", " : "", kMaterialKinds[k].section);
                for (size_t i = 0; i < t[k].recs.size(); ++i) {
                    uint32_t u[4];
                    std::memcpy(u, &t[k].recs[i], 16);
                    std::printf("%s[%u, %u, %u, %u]", i ? ", " : "", u[0], u[1], u[2], u[3]);
                }
                std::printf("], \"tri\": [");
                for (size_t i = 0; i < t[k].tri.size(); ++i) std::printf("%s%u", i ? ", " : "", t[k].tri[i]);
                std::printf("]}");
            }
            std::printf("]}\n");
        } else if (cmd == "residency") {
            const std::vector<uint8_t> r = plain_image_residency(scene, paired);
            std::printf("{\"resident\": [");
            for (size_t i = 0; i < r.size(); ++i) std::printf("%s%u", i ? ", " : "", (unsigned)r[i]);
            std::printf("]}\n");
        } else {
            std::fprintf(stderr, "unknown command: %s\n", cmd.c_str());
            return 2;
        }
        if (in.fail() && !in.eof()) { std::fprintf(stderr, "bad arguments: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
