// LocalFeaturesHip::verify_fundamental (include/local_features.hpp) from a program: reads two keypoint lists and the (i, j)
// matches, writes F and the inliers.  Usage: demo_verify_fundamental MODEL_DIR IN_PREFIX OUT_PREFIX
//   IN_PREFIX.ka / .kb: f32 rows of 5 (x, y, size, angle, response); IN_PREFIX.m: int32 (i, j) pairs
//   OUT_PREFIX.F: 9 f32 (nothing valid: not written); OUT_PREFIX.inl: int32 (i, j) pairs
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "local_features.hpp"

namespace lf = local_features;

template <typename T>
static std::vector<T> load(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> v(bytes.size() / sizeof(T));
    std::copy(bytes.begin(), bytes.begin() + v.size() * sizeof(T), reinterpret_cast<char *>(v.data()));
    return v;
}

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: demo_verify_fundamental MODEL_DIR IN_PREFIX OUT_PREFIX\n");
        return 2;
    }
    const std::string in = argv[2], out = argv[3];
    const std::vector<lf::Keypoint> ka = load<lf::Keypoint>(in + ".ka"), kb = load<lf::Keypoint>(in + ".kb");
    const std::vector<std::int32_t> raw = load<std::int32_t>(in + ".m");
    std::vector<std::pair<std::size_t, std::size_t>> matches, inliers;
    for (std::size_t i = 0; i + 1 < raw.size(); i += 2) matches.emplace_back(std::size_t(raw[i]), std::size_t(raw[i + 1]));
    try {
        lf::BuildTimeParams fixed;
        fixed.max_image_width = fixed.max_image_height = 64;
        fixed.max_features = 64;
        lf::LocalFeaturesHip feats = lf::new_hip(fixed, lf::FeatureDetectParams{}, argv[1]);
        float F[9];
        const bool found = feats.verify_fundamental(ka, kb, matches, F, inliers);
        if (found) std::ofstream(out + ".F", std::ios::binary).write(reinterpret_cast<const char *>(F), sizeof(F));
        std::vector<std::int32_t> flat;
        for (const auto &ij : inliers) {
            flat.push_back(std::int32_t(ij.first));
            flat.push_back(std::int32_t(ij.second));
        }
        std::ofstream(out + ".inl", std::ios::binary).write(reinterpret_cast<const char *>(flat.data()), flat.size() * 4);
        std::printf("found %d inliers %zu of %zu\n", int(found), inliers.size(), matches.size());
        // a match outside the keypoint lists is the caller's error
        try {
            std::vector<std::pair<std::size_t, std::size_t>> bad{{ka.size(), 0}};
            feats.verify_fundamental(ka, kb, bad, F, inliers);
            std::printf("bad match: accepted\n");
        } catch (const lf::LocalFeaturesError &e) {
            std::printf("bad match: %s\n", e.kind == lf::LocalFeaturesError::Kind::InvalidParameters ? "InvalidParameters" : "other");
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
