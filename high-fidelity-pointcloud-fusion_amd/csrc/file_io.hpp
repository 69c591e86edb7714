// csrc/file_io.hpp -- the PCD, CSV and PLY writers and the PLY reader of include/hfpf.h: host code only, no kernel and no HIP call.
// Of hfpf.hip, which includes it once, at its end, it uses fail() alone (hfpf_read_ply reports through the handle's error text).
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hfpf.h"

namespace {

// Formats rows [0,n) with `fmt_row` on several host threads (one contiguous chunk each) and writes the chunks in
// order: ASCII formatting, not I/O, dominates the reference's savePCDFileASCII-style outputs.
template <typename F>
bool write_rows_parallel(FILE* f, uint64_t n, size_t bytes_per_row_hint, F fmt_row)
{
    if (n == 0) return true;
    unsigned hw = std::thread::hardware_concurrency();
    const unsigned n_thr = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<unsigned>(hw ? hw : 1, 16), n / 4096 + 1));
    std::vector<std::string> parts(n_thr);
    std::vector<std::thread> thr;
    const uint64_t per = (n + n_thr - 1) / n_thr;
    for (unsigned t = 0; t < n_thr; t++) {
        thr.emplace_back([&, t] {
            const uint64_t a = t * per, b = std::min<uint64_t>(n, a + per);
            std::string& s = parts[t];
            if (b > a) s.reserve((size_t)(b - a) * bytes_per_row_hint);
            char line[256];
            for (uint64_t i = a; i < b; i++) {
                const int len = fmt_row(i, line, sizeof line);
                if (len > 0) s.append(line, (size_t)len);
            }
        });
    }
    for (auto& t : thr) t.join();
    for (auto& s : parts)
        if (!s.empty() && fwrite(s.data(), 1, s.size(), f) != s.size()) return false;
    return true;
}

}  // namespace

extern "C" {

int hfpf_write_pcd(const hfpf_row* rows, uint64_t n, const char* path)
{
    if (!path || (!rows && n)) return HFPF_ERR_BAD_ARG;
    FILE* f = fopen(path, "w");
    if (!f) return HFPF_ERR_IO;
    // PCL PCDWriter::writeASCII layout for PointXYZRGBNormal (pcl::io::savePCDFileASCII, grid.hpp:485), precision 8.
    fprintf(f, "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb normal_x normal_y normal_z curvature\n");
    fprintf(f, "SIZE 4 4 4 4 4 4 4 4\nTYPE F F F U F F F F\nCOUNT 1 1 1 1 1 1 1 1\n");
    fprintf(f, "WIDTH %llu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %llu\nDATA ascii\n", (unsigned long long)n, (unsigned long long)n);
    // the reference never writes rgb (grid.hpp:471-479): a default-constructed PCL point has r=g=b=0, a=255
    bool ok = write_rows_parallel(f, n, 96, [rows](uint64_t i, char* line, size_t cap) {
        const hfpf_row& r = rows[i];
        return snprintf(line, cap, "%.8g %.8g %.8g %u %.8g %.8g %.8g 0\n", r.x, r.y, r.z, 0xFF000000u | r.rgb, r.nx, r.ny, r.nz);
    });
    ok = ok && !ferror(f);
    return (fclose(f) == 0 && ok) ? HFPF_OK : HFPF_ERR_IO;
}

int hfpf_write_meta_csv(const hfpf_row* rows, uint64_t n, const char* path)
{
    if (!path || (!rows && n)) return HFPF_ERR_BAD_ARG;
    FILE* f = fopen(path, "w");
    if (!f) return HFPF_ERR_IO;
    fprintf(f, "Id,sdx,sdy,sdz,mean distance from normal, distance from normal sd, points in cylinder\n");  // grid.hpp:462 verbatim
    // default ostream float formatting = %g (6 significant digits), grid.hpp:478
    bool ok = write_rows_parallel(f, n, 80, [rows](uint64_t i, char* line, size_t cap) {
        const hfpf_row& r = rows[i];
        return snprintf(line, cap, "%llu,%g,%g,%g,%g,%g,%d\n", (unsigned long long)i, r.sdx, r.sdy, r.sdz, r.mean_dist, r.sd_dist, (int)r.count);
    });
    ok = ok && !ferror(f);
    return (fclose(f) == 0 && ok) ? HFPF_OK : HFPF_ERR_IO;
}

// downloadHQ / downloadClassified / download(XYZRGB) (grid.hpp:491-575; only referenced inside `#if 0`, node.cpp:399-437)
// as one writer over already extracted rows: PointXYZRGB cloud, optional count filter and colour coding.
int hfpf_write_pcd_xyzrgb(const hfpf_row* rows, uint64_t n, const char* path, uint32_t min_count, int32_t classify_threshold, int32_t white)
{
    if (!path || (!rows && n)) return HFPF_ERR_BAD_ARG;
    uint64_t kept = 0;
    for (uint64_t i = 0; i < n; i++) kept += rows[i].count >= min_count ? 1 : 0;  // `if(data->count<threshold) continue;` grid.hpp:561
    FILE* f = fopen(path, "w");
    if (!f) return HFPF_ERR_IO;
    fprintf(f, "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\n");
    fprintf(f, "WIDTH %llu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %llu\nDATA ascii\n", (unsigned long long)kept, (unsigned long long)kept);
    for (uint64_t i = 0; i < n; i++) {
        const hfpf_row& r = rows[i];
        if (r.count < min_count) continue;
        uint32_t rgb = white ? 0x00FFFFFFu : r.rgb;                                                // pt.r=g=b=255, grid.hpp:527-529,558-560
        if (classify_threshold >= 0 && (int64_t)r.count > (int64_t)classify_threshold) rgb = 0x00FF0000u;  // g=b=0, grid.hpp:530-534
        fprintf(f, "%.8g %.8g %.8g %u\n", r.x, r.y, r.z, 0xFF000000u | rgb);
    }
    const bool ok = !ferror(f);
    return (fclose(f) == 0 && ok) ? HFPF_OK : HFPF_ERR_IO;
}

// A mesh as binary little-endian PLY: 27 bytes a vertex (x y z nx ny nz as f32, red green blue), 13 a face (count 3, three u32).
int hfpf_write_ply(const hfpf_mesh_vertex* verts, uint64_t n_verts, const uint32_t* tris, uint64_t n_tris, const char* path)
{
    if (!path || (!verts && n_verts) || (!tris && n_tris)) return HFPF_ERR_BAD_ARG;
    FILE* f = fopen(path, "wb");
    if (!f) return HFPF_ERR_IO;
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %llu\nproperty float x\nproperty float y\nproperty float z\n"
               "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
               "element face %llu\nproperty list uchar uint vertex_indices\nend_header\n",
            (unsigned long long)n_verts, (unsigned long long)n_tris);
    constexpr uint64_t kChunk = 1u << 16;
    std::vector<uint8_t> buf(kChunk * 27);
    bool ok = true;
    for (uint64_t i0 = 0; i0 < n_verts && ok; i0 += kChunk) {
        const uint64_t n = std::min(kChunk, n_verts - i0);
        uint8_t* o = buf.data();
        for (uint64_t i = i0; i < i0 + n; i++, o += 27) {
            const hfpf_mesh_vertex& v = verts[i];
            memcpy(o, &v.x, 24);  // x y z nx ny nz
            o[24] = (uint8_t)(v.rgb >> 16), o[25] = (uint8_t)(v.rgb >> 8), o[26] = (uint8_t)v.rgb;
        }
        ok = fwrite(buf.data(), 27, n, f) == n;
    }
    for (uint64_t i0 = 0; i0 < n_tris && ok; i0 += kChunk) {
        const uint64_t n = std::min(kChunk, n_tris - i0);
        uint8_t* o = buf.data();
        for (uint64_t i = i0; i < i0 + n; i++, o += 13) {
            o[0] = 3;
            memcpy(o + 1, tris + 3 * i, 12);
        }
        ok = fwrite(buf.data(), 13, n, f) == n;
    }
    ok = ok && !ferror(f);
    return (fclose(f) == 0 && ok) ? HFPF_OK : HFPF_ERR_IO;
}

// The inverse of hfpf_write_ply (include/hfpf.h).  The header is parsed line by line; the vertex and face counts are checked against
// the bytes the file has left before anything is allocated.
int hfpf_read_ply(const char* path, hfpf_mesh_vertex** verts, uint64_t* n_verts, uint32_t** tris, uint64_t* n_tris)
{
    if (!path || !verts || !n_verts || !tris || !n_tris) return HFPF_ERR_BAD_ARG;
    *verts = nullptr, *tris = nullptr, *n_verts = 0, *n_tris = 0;
    FILE* f = fopen(path, "rb");
    if (!f) return fail(nullptr, HFPF_ERR_IO, "read_ply: cannot open %s", path);
    hfpf_mesh_vertex* hv = nullptr;
    uint32_t* ht = nullptr;
    auto bad = [&](const char* what) {
        fclose(f);
        free(hv), free(ht);
        return fail(nullptr, HFPF_ERR_IO, "read_ply: %s: %s", path, what);
    };
    if (fseek(f, 0, SEEK_END) != 0) return bad("not seekable");
    const long end = ftell(f);
    if (end < 0 || fseek(f, 0, SEEK_SET) != 0) return bad("not seekable");
    auto type_size = [](const char* t) -> int {
        static const struct { const char* name; int size; } kTypes[] = {{"char", 1}, {"int8", 1}, {"uchar", 1}, {"uint8", 1}, {"short", 2}, {"int16", 2},
            {"ushort", 2}, {"uint16", 2}, {"int", 4}, {"int32", 4}, {"uint", 4}, {"uint32", 4}, {"float", 4}, {"float32", 4}, {"double", 8}, {"float64", 8}};
        for (const auto& k : kTypes)
            if (strcmp(t, k.name) == 0) return k.size;
        return 0;
    };
    auto is_float = [](const char* t) { return strcmp(t, "float") == 0 || strcmp(t, "float32") == 0; };
    auto is_uchar = [](const char* t) { return strcmp(t, "uchar") == 0 || strcmp(t, "uint8") == 0; };
    char line[512];
    if (!fgets(line, sizeof line, f) || strncmp(line, "ply", 3) != 0) return bad("not a PLY file");
    int element = 0;  // 0 = none yet, 1 = vertex, 2 = face, 3 = one behind them
    bool format_ok = false, ended = false, face_list = false;
    unsigned long long nv = 0, nt = 0;
    int vsize = 0, off[9] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};  // x y z nx ny nz red green blue: byte offsets in a vertex record
    static const char* const kNames[9] = {"x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"};
    for (int n_lines = 0; n_lines < 4096 && fgets(line, sizeof line, f); n_lines++) {
        char a[64] = "", b[64] = "", c[64] = "", d[64] = "", e[64] = "";
        const int nf = sscanf(line, "%63s %63s %63s %63s %63s", a, b, c, d, e);
        if (nf < 1 || strcmp(a, "comment") == 0 || strcmp(a, "obj_info") == 0) continue;
        if (strcmp(a, "end_header") == 0) {
            ended = true;
            break;
        }
        if (strcmp(a, "format") == 0) {
            if (nf < 3 || strcmp(b, "binary_little_endian") != 0 || strcmp(c, "1.0") != 0) return bad("only format binary_little_endian 1.0 is read");
            format_ok = true;
        } else if (strcmp(a, "element") == 0) {
            char* tail = nullptr;
            const unsigned long long cnt = nf >= 3 ? strtoull(c, &tail, 10) : 0;
            if (nf < 3 || !tail || *tail || c[0] == '-') return bad("malformed element line");
            if (element == 0 && strcmp(b, "vertex") == 0) element = 1, nv = cnt;
            else if (element == 1 && strcmp(b, "face") == 0) element = 2, nt = cnt;
            else if (element >= 2) element = 3;
            else return bad("the vertex element must come first and the face element second");
        } else if (strcmp(a, "property") == 0) {
            if (element == 1) {
                const int sz = nf >= 3 ? type_size(b) : 0;
                if (!sz) return bad("a vertex property must be a scalar of a known type");
                for (int k = 0; k < 9; k++)
                    if (strcmp(c, kNames[k]) == 0 && (k < 6 ? is_float(b) : is_uchar(b))) off[k] = vsize;
                vsize += sz;
            } else if (element == 2) {
                const bool ok = nf >= 5 && strcmp(b, "list") == 0 && is_uchar(c) && (strcmp(d, "uint") == 0 || strcmp(d, "int") == 0 || strcmp(d, "uint32") == 0 ||
                                                                                    strcmp(d, "int32") == 0) &&
                                (strcmp(e, "vertex_indices") == 0 || strcmp(e, "vertex_index") == 0);
                if (!ok || face_list) return bad("the face element must be one property list uchar uint|int vertex_indices");
                face_list = true;
            } else if (element == 0) {
                return bad("a property outside an element");
            }
        } else {
            return bad("unknown header line");
        }
    }
    if (!ended || !format_ok) return bad("incomplete header");
    if (element < 1 || off[0] < 0 || off[1] < 0 || off[2] < 0) return bad("the vertex element needs float x, y, z");
    if (nt && !face_list) return bad("the face element has no vertex_indices list");
    const long at = ftell(f);
    if (at < 0) return bad("not seekable");
    const unsigned long long left = (unsigned long long)(end - at);
    if (nv >= 0xFFFFFFFFull || nt >= 0xFFFFFFFFull) return bad("more than 2^32 - 2 vertices or faces");
    if (nv * (unsigned long long)vsize > left || nt * 13ull > left - nv * (unsigned long long)vsize) return bad("the file is shorter than its header claims");
    hv = (hfpf_mesh_vertex*)malloc(std::max<size_t>((size_t)nv * sizeof(hfpf_mesh_vertex), 1));
    ht = (uint32_t*)malloc(std::max<size_t>((size_t)nt * 12, 1));
    if (!hv || !ht) return bad("out of memory");
    constexpr uint64_t kChunk = 1u << 14;
    std::vector<uint8_t> buf((size_t)kChunk * std::max(vsize, 13));
    for (uint64_t i0 = 0; i0 < nv; i0 += kChunk) {
        const uint64_t n = std::min<uint64_t>(kChunk, nv - i0);
        if (fread(buf.data(), (size_t)vsize, n, f) != n) return bad("truncated vertex data");
        for (uint64_t i = 0; i < n; i++) {
            const uint8_t* r = buf.data() + i * (size_t)vsize;
            hfpf_mesh_vertex v;
            memset(&v, 0, sizeof v);
            float* dst[6] = {&v.x, &v.y, &v.z, &v.nx, &v.ny, &v.nz};
            for (int k = 0; k < 6; k++)
                if (off[k] >= 0) memcpy(dst[k], r + off[k], 4);
            for (int k = 6; k < 9; k++)
                if (off[k] >= 0) v.rgb |= (uint32_t)r[off[k]] << (8 * (8 - k));
            hv[i0 + i] = v;
        }
    }
    for (uint64_t i0 = 0; i0 < nt; i0 += kChunk) {
        const uint64_t n = std::min<uint64_t>(kChunk, nt - i0);
        if (fread(buf.data(), 13, n, f) != n) return bad("truncated face data");
        for (uint64_t i = 0; i < n; i++) {
            const uint8_t* r = buf.data() + i * 13;
            if (r[0] != 3) return bad("a face that is not a triangle");
            memcpy(ht + 3 * (i0 + i), r + 1, 12);
        }
    }
    fclose(f);
    *verts = hv, *tris = ht, *n_verts = nv, *n_tris = nt;
    return HFPF_OK;
}

// Same fields as hfpf_write_pcd with DATA binary (40 bytes/point): for outputs where ASCII formatting would dominate.
int hfpf_write_pcd_binary(const hfpf_row* rows, uint64_t n, const char* path)
{
    if (!path || (!rows && n)) return HFPF_ERR_BAD_ARG;
    FILE* f = fopen(path, "wb");
    if (!f) return HFPF_ERR_IO;
    fprintf(f, "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb normal_x normal_y normal_z curvature\n");
    fprintf(f, "SIZE 4 4 4 4 4 4 4 4\nTYPE F F F U F F F F\nCOUNT 1 1 1 1 1 1 1 1\n");
    fprintf(f, "WIDTH %llu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %llu\nDATA binary\n", (unsigned long long)n, (unsigned long long)n);
    std::vector<char> buf;
    buf.reserve(32 * 4096);
    for (uint64_t i = 0; i < n; i++) {
        const hfpf_row& r = rows[i];
        const float zero = 0.f;
        const uint32_t rgba = 0xFF000000u | r.rgb;
        const void* fields[8] = {&r.x, &r.y, &r.z, &rgba, &r.nx, &r.ny, &r.nz, &zero};
        for (int k = 0; k < 8; k++) buf.insert(buf.end(), (const char*)fields[k], (const char*)fields[k] + 4);
        if (buf.size() >= 32 * 4096 || i + 1 == n) {
            fwrite(buf.data(), 1, buf.size(), f);
            buf.clear();
        }
    }
    const bool ok = !ferror(f);
    return (fclose(f) == 0 && ok) ? HFPF_OK : HFPF_ERR_IO;
}

}  // extern "C"
