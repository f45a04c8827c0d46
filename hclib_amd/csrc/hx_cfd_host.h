// hx_cfd_host.h — the reader of a Rodinia CFD mesh file, plain C++ (no HIP):
// euler3d_cpu_double.ref.cpp:417-455 through the same std::ifstream
// extractions, so a number is a number here exactly where it is one there.
// What the reference does not check is refused: a stream that fails (a missing
// file, a truncated one, a token that is no number) and nel < 1.
#pragma once

#include <fstream>
#include <string>

#include "hx_cfd_plan.h"

namespace hx {

// With every array null: only nel and nelr. Otherwise the arrays hold nelr
// rows (nelr, nelr * 4, nelr * 12 entries) and nel_expected is what a first
// call reported. 0, or -1 with `err`.
inline int cfd_read_input(const char *path, int nel_expected, double *areas, int *neighbours, double *normals,
                          int &nel, int &nelr, std::string &err) {
    auto fail = [&](const std::string &m) {
        err = m;
        return -1;
    };
    if (!path) return fail("the path must not be NULL");
    const bool fill = areas || neighbours || normals;
    if (fill && !(areas && neighbours && normals)) return fail("the arrays must be all NULL or none");
    std::ifstream file(path);
    if (!file) return fail(std::string("cannot open ") + path);
    int n = 0;
    file >> n;
    if (file.fail()) return fail(std::string(path) + ": no element count");
    if (n < 1) return fail(std::string(path) + ": nel must be at least 1 (nel " + std::to_string(n) + ")");
    if (n > (INT32_MAX - 7) / (kCfdNnb * kCfdNdim))
        return fail(std::string(path) + ": nel " + std::to_string(n) + " is above what the reference's int indices reach");
    nel = n;
    nelr = (int)cfd_nelr(n);
    if (!fill) return 0;
    if (n != nel_expected) return fail(std::string(path) + ": the element count differs from the first call's");
    auto bad = [&](int i) { return fail(std::string(path) + ": truncated or not a number at element " + std::to_string(i)); };
    for (int i = 0; i < nel; i++) {
        file >> areas[i];
        for (int j = 0; j < kCfdNnb; j++) {
            int &e = neighbours[i * kCfdNnb + j];
            file >> e;
            if (file.fail()) return bad(i);
            if (e < 0) e = -1;
            e--;  // Fortran numbering
            for (int k = 0; k < kCfdNdim; k++) {
                double &v = normals[(i * kCfdNnb + j) * kCfdNdim + k];
                file >> v;
                v = -v;
            }
        }
        if (file.fail()) return bad(i);
    }
    // the padding: copies of the last element
    const int last = nel - 1;
    for (int i = nel; i < nelr; i++) {
        areas[i] = areas[last];
        for (int j = 0; j < kCfdNnb; j++) {
            neighbours[i * kCfdNnb + j] = neighbours[last * kCfdNnb + j];
            for (int k = 0; k < kCfdNdim; k++)
                normals[(i * kCfdNnb + j) * kCfdNdim + k] = normals[(last * kCfdNnb + j) * kCfdNdim + k];
        }
    }
    return 0;
}

}  // namespace hx
