// index_io.cpp — the file frame of the indexes (index_io.h).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "index_io.h"
#include "weights.h"

namespace bert_hip {

bool device_to_file(FILE *f, const void *d, size_t bytes, size_t piece, std::vector<char> &buf, std::string &err) {
    for (size_t o = 0; o < bytes; o += piece) {
        const size_t c = std::min(piece, bytes - o);
        if (buf.size() < c) buf.resize(c);
        HIP_OK(hipMemcpy(buf.data(), (const char *)d + o, c, hipMemcpyDeviceToHost), err, false);
        if (fwrite(buf.data(), 1, c, f) != c) { err = "write failed"; return false; }
    }
    return true;
}

bool file_to_device(FILE *f, void *d, size_t bytes, size_t piece, std::vector<char> &buf, std::string &err) {
    for (size_t o = 0; o < bytes; o += piece) {
        const size_t c = std::min(piece, bytes - o);
        if (buf.size() < c) buf.resize(c);
        if (fread(buf.data(), 1, c, f) != c) { err = "read failed"; return false; }
        HIP_OK(hipMemcpy((char *)d + o, buf.data(), c, hipMemcpyHostToDevice), err, false);
    }
    return true;
}

bool write_atomically(const char *path, std::string &err, const std::function<bool(FILE *)> &body) {
    const std::string tmp = std::string(path) + ".tmp";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) { err = "cannot write '" + tmp + "'"; return false; }
    bool ok = body(f);
    ok = (fclose(f) == 0) && ok;
    if (ok && rename(tmp.c_str(), path) != 0) ok = false;
    if (!ok) {
        (void)::remove(tmp.c_str());
        if (err.empty()) err = "cannot write '" + std::string(path) + "'";
    }
    return ok;
}

}  // namespace bert_hip
