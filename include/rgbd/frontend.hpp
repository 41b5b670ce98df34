// rgbd/frontend.hpp -- header-only C++ surfaces over the C ABI, named and shaped like the
// reference's classes so System/Tracking.cpp-style callers port line for line:
//
//   rgbd::ORBextractor   <- ORBextractor / Extractor(ORB2, ORB2, NORMAL)  Features/ORBextractor.h:9-66
//   rgbd::Extractor      <- Extractor(detector, descriptor, mode): (ORB2, ORB2) or (SVO, BRIEF), NORMAL
//                           (main.cpp:31's default)                       Features/Extractor.h:9-72
//   rgbd::Frame          <- Frame (keys, keysUn, descriptors, keys3Dc, outlier flags, pose)  Core/Frame.h
//   rgbd::Matcher        <- Matcher::match, Matcher::projectionMatch      Features/Matcher.h:23-26
//   rgbd::RansacSE3      <- RansacSE3::compute + rmse / mvInliers / mT21   Solver/SolverSE3.h:15-57
//   rgbd::Gicp           <- Gicp::compute / align + setters                 Solver/Gicp.h:10-57
//   rgbd::PnPRansac      <- PnPRansac::compute                             Solver/PnPRansac.h
//   rgbd::Vocabulary     <- DBoW3::Vocabulary (transform, score, size; TF_IDF + L1_NORM)  Core/Frame.cpp:243-249
//   rgbd::LoopDetector   <- LoopDetector::add / obtainCandidates            PlaceRecognition/LoopDetector.cpp:22-84
//   rgbd::OctomapDrawer  <- OctomapDrawer::reset / insertCloud + the leaves render draws  Drawer/OctomapDrawer.cpp:15-79
//
// No OpenCV/Eigen types: poses are row-major float[16] (cv::Mat 4x4 CV_32F layout), keypoints and
// matches are the byte-identical rgbd_keypoint / rgbd_dmatch.  INTEGRATION.md shows the thin
// cv::Feature2D / cv::Mat adapters a maintainer adds on the reference side.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../rgbd_hip.h"

namespace rgbd {

class Error : public std::runtime_error {
public:
    using std::runtime_error::runtime_error;
};

inline void check(rgbd_ctx* c, rgbd_status s, const char* what)
{
    if (s != RGBD_OK) throw Error(std::string(what) + ": " + rgbd_last_error(c));
}

using Pose = std::array<float, 16>;
inline Pose identity() { return Pose{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}; }

// One extraction context (device workspace + camera); what Frame needs from an extractor.
class ExtractorBase {
public:
    // Extractor::detectAndCompute (mask ignored, as in the reference)
    void detectAndCompute(const uint8_t* gray, int step, std::vector<rgbd_keypoint>& kps,
                          std::vector<uint8_t>& desc)
    {
        const int cap = rgbd_max_keypoints(ctx_.get());
        kps.resize(cap);
        desc.resize((size_t)cap * 32);
        int n = 0;
        check(ctx_.get(), rgbd_detect_and_compute(ctx_.get(), gray, step, kps.data(), desc.data(), cap, &n),
              "detectAndCompute");
        kps.resize(n);
        desc.resize((size_t)n * 32);
    }
    rgbd_ctx* ctx() const { return ctx_.get(); }
    const rgbd_camera& camera() const { return cam_; }

protected:
    void adopt(rgbd_ctx* c, rgbd_status s, const rgbd_camera& cam, const char* what)
    {
        cam_ = cam;
        ctx_.reset(c, rgbd_destroy);
        check(c, s, what);
    }
    std::shared_ptr<rgbd_ctx> ctx_;
    rgbd_camera cam_{};
};

// Shared by every Frame of a sequence (main.cpp:31 shares one Extractor); one per thread.
class ORBextractor : public ExtractorBase {
public:
    ORBextractor(int width, int height, const rgbd_camera& cam, int nfeatures = 1000, float scaleFactor = 1.2f,
                 int nlevels = 8, int iniThFAST = 20, int minThFAST = 7, int device = 0, int max_batch = 1)
    {
        rgbd_orb_params p{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST};
        rgbd_ctx* c = nullptr;
        const rgbd_status s = rgbd_create(device, width, height, max_batch, &p, &cam, &c);
        adopt(c, s, cam, "rgbd_create");
    }
};

// Extractor(eType detector, eType descriptor, eMode mode) -- Features/Extractor.cpp:15-22.  The accelerated
// pairs are (ORB2, ORB2), (SVO, BRIEF) (main.cpp:31 runs the latter), (GFTT, BRIEF) (cv::GFTTDetector, :178-181),
// (FAST, BRIEF) and (FAST, ORB) (cv::FastFeatureDetector::create(), :168-171, with BRIEF or cv::ORB::create() as
// descriptor) and (ORB, ORB) (cv::ORB as detector and descriptor, :163-166, 216-218) in NORMAL mode and (FAST, BRIEF) in ADAPTIVE mode (createAdaptiveDetector, :82-109); the other OpenCV stock
// detectors / descriptors and the other ADAPTIVE adjusters (GFTT, ORB, SURF, SIFT) are not on this path and throw.
class Extractor : public ExtractorBase {
public:
    enum eType { ORB = 0, ORB2, SVO, FAST, GFTT, STAR, BRISK, FREAK, BRIEF, LATCH, SURF, SIFT };
    enum eMode { NORMAL = 0, ADAPTIVE };

    Extractor(eType detector, eType descriptor, eMode mode, int width, int height, const rgbd_camera& cam,
              int device = 0, int max_batch = 1)
        : mDetectorType(detector), mDescriptorType(descriptor), mMode(mode), W_(width), H_(height),
          device_(device), maxB_(max_batch)
    {
        const bool orb2 = detector == ORB2 && descriptor == ORB2, svo = detector == SVO && descriptor == BRIEF;
        const bool adaptive = mode == ADAPTIVE && detector == FAST && descriptor == BRIEF;
        const bool gftt = detector == GFTT && descriptor == BRIEF;
        const bool cvorb = detector == ORB && descriptor == ORB;
        const bool fast = detector == FAST && (descriptor == BRIEF || descriptor == ORB);
        if (!adaptive && (mode != NORMAL || !(orb2 || svo || gftt || cvorb || fast)))
            throw Error("Extractor: only (ORB2, ORB2), (SVO, BRIEF), (GFTT, BRIEF), (FAST, BRIEF), (FAST, ORB) and (ORB, ORB) in NORMAL mode and (FAST, BRIEF) in ADAPTIVE mode are accelerated");
        cam_ = cam;
        setParameters(1000, 1.2f, 8, 20, 7);   // :21
    }
    // Extractor::setParameters (:24-48): recreates the context
    void setParameters(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
    {
        nfeatures_ = nfeatures;
        scale_ = scaleFactor;
        nlevels_ = nlevels;
        rgbd_ctx* c = nullptr;
        rgbd_status s;
        if (mMode == ADAPTIVE) {
            // createAdaptiveDetector (:82-109): DetectorAdjuster(FAST, 20, 2, 10000, 1.3, 0.7), 600 minimum
            // features, 5 iterations, a 3 x 3 grid with edge threshold 31; nlevels and scaleFactor only shape
            // init()'s tables, which the getters below report
            rgbd_adaptive_params p{nfeatures, 600, 3, 3, 31, 5, 0, 0, 20.0, 2.0, 10000.0, 1.3, 0.7};
            s = rgbd_create_adaptive(device_, W_, H_, maxB_, &p, &cam_, &c);
        } else if (mDetectorType == FAST) {
            // cv::FastFeatureDetector::create(), :168-171: threshold 10, nonmaxSuppression, TYPE_9_16; the corner list
            // at its largest (65536), the default output slack
            rgbd_fast_params p{nfeatures, 10, mDescriptorType == ORB ? RGBD_FAST_ORB : RGBD_FAST_BRIEF, 65536, 0};
            s = rgbd_create_fast(device_, W_, H_, maxB_, &p, &cam_, &c);
        } else if (mDetectorType == GFTT) {
            // GFTTDetector::create(nfeatures, 0.01, 3, 3, false, 0.04), :178-181: nfeatures is maxCorners
            rgbd_gftt_params p{nfeatures, 0, 0.01, 3.0};
            s = rgbd_create_gftt(device_, W_, H_, maxB_, &p, &cam_, &c);
        } else if (mDetectorType == ORB) {
            // cv::ORB::create(nfeatures, scaleFactor, nlevels), :163-166: edgeThreshold 31, fastThreshold 20; the
            // corner lists at their largest (12288 per level), the default output slack
            rgbd_cvorb_params p{nfeatures, scaleFactor, nlevels, 31, 20, 12288, 0};
            s = rgbd_create_cvorb(device_, W_, H_, maxB_, &p, &cam_, &c);
        } else if (mDetectorType == SVO) {
            rgbd_svo_params p{nfeatures, nlevels, 5, 20, 0};   // SVOextractor(nlevels, 5, 20), :162-165
            s = rgbd_create_svo(device_, W_, H_, maxB_, &p, &cam_, &c);
        } else {
            rgbd_orb_params p{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST};
            s = rgbd_create(device_, W_, H_, maxB_, &p, &cam_, &c);
        }
        adopt(c, s, cam_, "Extractor");
    }
    // getters (:97-151); the SVO, GFTT, ORB and ADAPTIVE branches report init()'s tables, the ORB2 branch ORBextractor's
    // (same values)
    int getLevels() const { return nlevels_; }
    float getScaleFactor() const { return scale_; }
    std::vector<float> getScaleFactors() const
    {
        std::vector<float> f((size_t)nlevels_, 1.0f);
        for (int i = 1; i < nlevels_; i++) f[i] = f[i - 1] * scale_;
        return f;
    }
    std::vector<float> getInverseScaleFactors() const
    {
        std::vector<float> f = getScaleFactors();
        for (float& v : f) v = 1.0f / v;
        return f;
    }
    std::vector<float> getScaleSigmaSquares() const
    {
        std::vector<float> f = getScaleFactors();
        for (float& v : f) v = v * v;
        return f;
    }
    std::vector<float> getInverseScaleSigmaSquares() const
    {
        std::vector<float> f = getScaleSigmaSquares();
        for (float& v : f) v = 1.0f / v;
        return f;
    }
    // OpenCV's own BRIEF tests (opencv_contrib generated_32.i), 256 x {y1, x1, y2, x2}; SVO, GFTT, (FAST, BRIEF) and ADAPTIVE contexts only
    void setBriefPattern(const int8_t* pairs) { check(ctx_.get(), rgbd_svo_set_brief_pattern(ctx_.get(), pairs), "setBriefPattern"); }

    eType mDetectorType, mDescriptorType;
    eMode mMode;

private:
    int W_, H_, device_, maxB_;
    int nfeatures_ = 1000, nlevels_ = 8;
    float scale_ = 1.2f;
};

using BowVector = std::map<uint32_t, double>;                       // DBoW3::BowVector: word id -> value
using FeatureVector = std::map<uint32_t, std::vector<unsigned>>;    // DBoW3::FeatureVector: node id -> feature indices

// DBoW3::Vocabulary over the device operator (DESIGN.md "Bag-of-words and loop detection definition").  The tree is
// uploaded to the context once; transform and score run on the device.
class Vocabulary {
public:
    // node arrays as rgbd_voc_set takes them (node 0 the root)
    Vocabulary(rgbd_ctx* ctx, int k, int L, const std::vector<int32_t>& parent, const std::vector<uint8_t>& descriptor,
               const std::vector<double>& weight, const std::vector<uint8_t>& is_leaf, const std::vector<int32_t>& word_id,
               int weighting = RGBD_VOC_TF_IDF, int scoring = RGBD_VOC_L1_NORM)
        : ctx_(ctx)
    {
        words_ = 0;
        for (uint8_t l : is_leaf) words_ += l ? 1u : 0u;
        check(ctx, rgbd_voc_set(ctx, k, L, weighting, scoring, 32, (int64_t)parent.size(), parent.data(), descriptor.data(),
                                weight.data(), is_leaf.data(), word_id.data()), "Vocabulary");
    }
    // DBoW3's text YAML, uncompressed (the layout recalled in rgbd-slam_amd/vocabulary.py, unpinned)
    static std::shared_ptr<Vocabulary> load(rgbd_ctx* ctx, const std::string& path)
    {
        FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) throw Error("Vocabulary: cannot open " + path);
        std::string text;
        char buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
        std::fclose(f);
        auto num = [&](const char* key, size_t from) -> double {
            const size_t at = text.find(key, from);
            if (at == std::string::npos) throw Error(std::string("Vocabulary: no ") + key);
            return std::strtod(text.c_str() + at + std::strlen(key), nullptr);
        };
        const int k = (int)num(" k:", 0), L = (int)num(" L:", 0);
        const int scoring = (int)num("scoringType:", 0), weighting = (int)num("weightingType:", 0);
        const size_t words_at = text.find("words:");
        if (words_at == std::string::npos) throw Error("Vocabulary: no words list");
        std::vector<int32_t> parent(1, 0), word(1, -1);
        std::vector<uint8_t> desc(32, 0), leaf(1, 0);
        std::vector<double> weight(1, 0.0);
        for (size_t at = text.find("nodeId:"); at != std::string::npos && at < words_at; at = text.find("nodeId:", at + 1)) {
            const size_t id = (size_t)num("nodeId:", at);
            if (id >= parent.size()) {
                parent.resize(id + 1, 0); word.resize(id + 1, -1); leaf.resize(id + 1, 0); weight.resize(id + 1, 0.0);
                desc.resize((id + 1) * 32, 0);
            }
            parent[id] = (int32_t)num("parentId:", at);
            weight[id] = num("weight:", at);
            const size_t d = text.find("dbw3", at);
            if (d == std::string::npos) throw Error("Vocabulary: a node without a descriptor");
            char* q = nullptr;
            const long type = std::strtol(text.c_str() + d + 4, &q, 10), cols = std::strtol(q, &q, 10);
            if (type != 0 || cols != 32) throw Error("Vocabulary: not a 32-byte CV_8U descriptor");
            for (int b = 0; b < 32; b++) desc[id * 32 + b] = (uint8_t)std::strtol(q, &q, 10);
        }
        for (size_t at = text.find("wordId:", words_at); at != std::string::npos; at = text.find("wordId:", at + 1)) {
            const size_t node = (size_t)num("nodeId:", at);
            if (node >= parent.size()) throw Error("Vocabulary: a word on an unknown node");
            leaf[node] = 1;
            word[node] = (int32_t)num("wordId:", at);
        }
        return std::make_shared<Vocabulary>(ctx, k, L, parent, desc, weight, leaf, word, weighting, scoring);
    }
    unsigned size() const { return words_; }
    rgbd_ctx* ctx() const { return ctx_; }
    // transform(features, BowVector, FeatureVector, levelsup) of n descriptors (n x 32 bytes)
    void transform(const uint8_t* desc, int n, BowVector& v, FeatureVector& fv, int levelsup) const
    {
        const size_t m = (size_t)std::max(n, 1);
        std::vector<uint32_t> ids(m);
        std::vector<double> vals(m);
        std::vector<int32_t> node(m), idx(m);
        int32_t nw = 0, nf = 0;
        check(ctx_, rgbd_bow_transform(ctx_, desc, n, levelsup, ids.data(), vals.data(), &nw, node.data(), idx.data(), &nf),
              "Vocabulary::transform");
        v.clear();
        fv.clear();
        for (int i = 0; i < nw; i++) v.emplace_hint(v.end(), ids[i], vals[i]);
        for (int i = 0; i < nf; i++) fv[(uint32_t)node[i]].push_back((unsigned)idx[i]);
    }
    double score(const BowVector& a, const BowVector& b) const
    {
        std::vector<uint32_t> ia, ib;
        std::vector<double> va, vb;
        flatten(a, ia, va);
        flatten(b, ib, vb);
        double s = 0.0;
        check(ctx_, rgbd_bow_score(ctx_, ia.data(), va.data(), (int32_t)ia.size(), ib.data(), vb.data(), (int32_t)ib.size(), &s),
              "Vocabulary::score");
        return s;
    }
    static void flatten(const BowVector& v, std::vector<uint32_t>& ids, std::vector<double>& vals)
    {
        ids.clear();
        vals.clear();
        for (const auto& kv : v) {
            ids.push_back(kv.first);
            vals.push_back(kv.second);
        }
    }

private:
    rgbd_ctx* ctx_;
    unsigned words_ = 0;
};

class Frame {
public:
    using Ptr = std::shared_ptr<Frame>;
    // Frame(imRGB, imDepth, ts, Extractor, RGBDcamera*) -- Core/Frame.cpp:34-73
    Frame(const uint8_t* bgr, const uint16_t* depth, double timeStamp, const ExtractorBase& ex)
        : mTimeStamp(timeStamp), mCamera(ex.camera())
    {
        mnId = nextId()++;                                           // Core/Frame.cpp: mnId = nNextId++
        rgbd_ctx* c = ex.ctx();
        const int cap = rgbd_max_keypoints(c);
        mvKeys.resize(cap);
        mvKeysUn.resize(cap);
        mDescriptors.resize((size_t)cap * 32);
        mvKeys3Dc.resize((size_t)cap * 3);
        int n = 0;
        check(c, rgbd_frame(c, bgr, depth, mvKeys.data(), mvKeysUn.data(), mDescriptors.data(), mvKeys3Dc.data(),
                            cap, &n), "Frame");
        N = n;
        mvKeys.resize(n);
        mvKeysUn.resize(n);
        mDescriptors.resize((size_t)n * 32);
        mvKeys3Dc.resize((size_t)n * 3);
        mvbOutlier.assign(n, 0);
        // computeImageBounds + the grid element sizes + assignFeaturesToGrid (Core/Frame.cpp:57-66, :75-89)
        rgbd_bounds b{};
        check(c, rgbd_image_bounds(c, &b), "image bounds");
        mnMinX = b.min_x; mnMaxX = b.max_x; mnMinY = b.min_y; mnMaxY = b.max_y;
        mfGridElementWidthInv = static_cast<float>(FRAME_GRID_COLS) / (mnMaxX - mnMinX);
        mfGridElementHeightInv = static_cast<float>(FRAME_GRID_ROWS) / (mnMaxY - mnMinY);
        mGrid.assign((size_t)FRAME_GRID_COLS * FRAME_GRID_ROWS, std::vector<size_t>());
        for (int i = 0; i < N; i++) {
            int gx, gy;
            if (posInGrid(mvKeysUn[i], gx, gy)) mGrid[(size_t)gx * FRAME_GRID_ROWS + gy].push_back((size_t)i);
        }
    }
    // Frame::posInGrid (Core/Frame.cpp:231-241); a keypoint outside the grid is in no cell
    bool posInGrid(const rgbd_keypoint& kp, int& posX, int& posY) const
    {
        const float fx = std::round((kp.x - mnMinX) * mfGridElementWidthInv);
        const float fy = std::round((kp.y - mnMinY) * mfGridElementHeightInv);
        if (!(fx >= 0.0f && fx < (float)FRAME_GRID_COLS && fy >= 0.0f && fy < (float)FRAME_GRID_ROWS)) return false;
        posX = (int)fx;
        posY = (int)fy;
        return true;
    }
    // Frame::getFeaturesInArea (Core/Frame.cpp:179-229), host code over mGrid; levels are checked when
    // minLevel > 0 || maxLevel >= 0, as in the reference
    std::vector<size_t> getFeaturesInArea(float x, float y, float r, int minLevel = -1, int maxLevel = -1) const
    {
        std::vector<size_t> vIndices;
        const float c0 = std::floor((x - mnMinX - r) * mfGridElementWidthInv), c1 = std::ceil((x - mnMinX + r) * mfGridElementWidthInv);
        const float r0 = std::floor((y - mnMinY - r) * mfGridElementHeightInv), r1 = std::ceil((y - mnMinY + r) * mfGridElementHeightInv);
        if (!(c0 < (float)FRAME_GRID_COLS) || !(c1 >= 0.0f) || !(r0 < (float)FRAME_GRID_ROWS) || !(r1 >= 0.0f)) return vIndices;
        const int nMinCellX = c0 > 0.0f ? (int)c0 : 0, nMaxCellX = c1 < (float)(FRAME_GRID_COLS - 1) ? (int)c1 : FRAME_GRID_COLS - 1;
        const int nMinCellY = r0 > 0.0f ? (int)r0 : 0, nMaxCellY = r1 < (float)(FRAME_GRID_ROWS - 1) ? (int)r1 : FRAME_GRID_ROWS - 1;
        const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
        for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
            for (int iy = nMinCellY; iy <= nMaxCellY; iy++)
                for (size_t j : mGrid[(size_t)ix * FRAME_GRID_ROWS + iy]) {
                    const rgbd_keypoint& kpUn = mvKeysUn[j];
                    if (bCheckLevels) {
                        if (kpUn.octave < minLevel) continue;
                        if (maxLevel >= 0 && kpUn.octave > maxLevel) continue;
                    }
                    if (std::fabs(kpUn.x - x) < r && std::fabs(kpUn.y - y) < r) vIndices.push_back(j);
                }
        return vIndices;
    }
    bool isValidObs(size_t i) const { return mvKeys3Dc[3 * i + 2] > 0; }      // Core/Frame.cpp:415-418
    bool isOutlier(size_t i) const { return mvbOutlier[i] != 0; }
    void setPose(const Pose& T) { mTcw = T; }
    const Pose& getPose() const { return mTcw; }
    std::vector<float> depths() const
    {
        std::vector<float> z(N);
        for (int i = 0; i < N; i++) z[i] = mvKeys3Dc[3 * (size_t)i + 2];
        return z;
    }
    // Frame::computeBoW (Core/Frame.cpp:243-249): once per frame, levelsup 4
    void computeBoW(const Vocabulary& voc)
    {
        if (mBowVec.empty()) voc.transform(mDescriptors.data(), N, mBowVec, mFeatVec, 4);
    }
    // Tracking::createKeyFrame's cloud (System/Tracking.cpp:234-237) from the keyframe's own images, camera frame
    void createFilteredCloud(const ExtractorBase& ex, const uint8_t* bgr, const uint16_t* depth)
    {
        const rgbd_cloud_params prm{6, 0.5f, 4.0f, 0.04f, 50, 1.0};
        mCloud.resize(16384);
        int32_t n = 0;
        check(ex.ctx(), rgbd_keyframe_cloud(ex.ctx(), bgr, depth, &prm, mCloud.data(), (int32_t)mCloud.size(), &n), "createFilteredCloud");
        mCloud.resize((size_t)n);
    }
    bool isValidCloud() const { return !mCloud.empty(); }
    int id() const { return mnId; }
    static int& nextId() { static int next = 0; return next; }      // Frame::nNextId
    // connections are kept as plain pointers: the map that owns the keyframes outlives them
    void addConnection(Frame* kf) { mspConnectedKFs.insert(kf); }
    const std::set<Frame*>& getConnectedKFs() const { return mspConnectedKFs; }

    static constexpr int FRAME_GRID_COLS = 64, FRAME_GRID_ROWS = 48;   // Core/Frame.h
    int N = 0;
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;   // undistorted image bounds (computeImageBounds)
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    std::vector<std::vector<size_t>> mGrid;                 // mGrid[ix * FRAME_GRID_ROWS + iy], ascending indices
    double mTimeStamp = 0;
    rgbd_camera mCamera{};                  // mpCamera (RGBDcamera)
    std::vector<rgbd_keypoint> mvKeys, mvKeysUn;
    std::vector<uint8_t> mDescriptors;      // N x 32
    std::vector<float> mvKeys3Dc;           // N x 3
    std::vector<uint8_t> mvbOutlier;
    Pose mTcw = identity();
    int mnId = 0;
    BowVector mBowVec;
    FeatureVector mFeatVec;
    double mScore = 0.0;
    std::set<Frame*> mspConnectedKFs;
    std::vector<rgbd_point> mCloud;         // mpCloud: the keyframe's filtered cloud (createFilteredCloud)
};

// OctomapDrawer over a device-resident occupancy map on the extractor's context: insertCloud is Frame::updateSensor
// (rgbd_occmap_sensor_pose) plus one scan of the keyframe's cloud; leaves is the query render draws from.  The leaves
// only: no inner nodes, no .ot file, no GL (DESIGN.md "Occupancy map definition"; parity with liboctomap is unpinned).
class OctomapDrawer {
public:
    explicit OctomapDrawer(rgbd_ctx* ctx, int64_t capacity = (int64_t)1 << 20) : ctx_(ctx)
    {
        const rgbd_occmap_params prm{0.08, 0.9, 0.4, 0.001, 0.999, capacity};   // OctomapDrawer::reset's values
        check(ctx_, rgbd_occmap_create(ctx_, &prm, &map_), "OctomapDrawer");
    }
    ~OctomapDrawer() { rgbd_occmap_destroy(map_); }
    OctomapDrawer(const OctomapDrawer&) = delete;
    OctomapDrawer& operator=(const OctomapDrawer&) = delete;
    void reset()
    {
        msIdxs.clear();
        check(ctx_, rgbd_occmap_clear(map_), "OctomapDrawer::reset");
    }
    // a keyframe id is inserted once; a cloud that does not fit the table throws and leaves the map as it was
    void insertCloud(Frame& KF, double maxRange = -1.0)
    {
        if (msIdxs.count(KF.id()) > 0) return;
        float Twc34[12], origin[3];
        if (rgbd_occmap_sensor_pose(KF.getPose().data(), Twc34, origin) != RGBD_OK) throw Error("OctomapDrawer::insertCloud: pose not finite");
        check(ctx_, rgbd_occmap_insert(map_, KF.mCloud.data(), (int32_t)KF.mCloud.size(), Twc34, origin, maxRange), "OctomapDrawer::insertCloud");
        msIdxs.insert(KF.id());
    }
    size_t size() const
    {
        int64_t n = 0;
        check(ctx_, rgbd_occmap_size(map_, &n), "OctomapDrawer::size");
        return (size_t)n;
    }
    // the leaves with occupancy >= minOccupancy (render's occThresh is 0.9; <= 0: all), ascending by key
    size_t leaves(std::vector<uint16_t>& keys, std::vector<float>& logodds, std::vector<uint8_t>& rgb, double minOccupancy = 0.0) const
    {
        const float lo = minOccupancy > 0.0 ? (float)std::log(minOccupancy / (1.0 - minOccupancy)) : -std::numeric_limits<float>::infinity();
        const size_t cap = std::max<size_t>(size(), 1);
        keys.resize(3 * cap);
        logodds.resize(cap);
        rgb.resize(3 * cap);
        int64_t n = 0;
        check(ctx_, rgbd_occmap_leaves(map_, lo, keys.data(), logodds.data(), rgb.data(), (int64_t)cap, &n), "OctomapDrawer::leaves");
        keys.resize(3 * (size_t)n);
        logodds.resize((size_t)n);
        rgb.resize(3 * (size_t)n);
        return (size_t)n;
    }

private:
    rgbd_ctx* ctx_;
    rgbd_occmap* map_ = nullptr;
    std::set<int> msIdxs;
};

// LoopDetector over the context's keyframe database: add uploads the keyframe's BoW vector; obtainCandidates scores
// the query against every entry on the device (two launches, one per argument order) and applies the reference's
// candidate rules on the host (rgbd_loop_candidates).
class LoopDetector {
public:
    explicit LoopDetector(std::shared_ptr<Vocabulary> voc, int interval = 10) : voc_(std::move(voc)), mnInterval(interval)
    {
        check(voc_->ctx(), rgbd_loopdb_clear(voc_->ctx()), "LoopDetector");
    }
    void add(const Frame::Ptr& pKF)
    {
        std::vector<uint32_t> ids;
        std::vector<double> vals;
        Vocabulary::flatten(pKF->mBowVec, ids, vals);
        int32_t e = 0;
        check(voc_->ctx(), rgbd_loopdb_add(voc_->ctx(), ids.data(), vals.data(), (int32_t)ids.size(), &e), "LoopDetector::add");
        entries_.push_back(pKF);
    }
    std::vector<Frame::Ptr> obtainCandidates(const Frame::Ptr& pKF)
    {
        std::vector<Frame::Ptr> out;
        const std::set<Frame*>& conn = pKF->getConnectedKFs();
        if (conn.empty()) return out;
        rgbd_ctx* c = voc_->ctx();
        const int32_t E = (int32_t)entries_.size();
        std::vector<uint32_t> ids;
        std::vector<double> vals;
        Vocabulary::flatten(pKF->mBowVec, ids, vals);
        std::vector<double> rev((size_t)std::max(E, 1)), score(rev.size());
        std::vector<int32_t> shared(rev.size()), first(rev.size()), fid(rev.size());
        std::vector<uint8_t> skip(rev.size(), 0);
        int32_t n = 0;
        check(c, rgbd_loopdb_query(c, ids.data(), vals.data(), (int32_t)ids.size(), 0, E, rev.data(), shared.data(), first.data(), &n),
              "LoopDetector::obtainCandidates");
        check(c, rgbd_loopdb_query(c, ids.data(), vals.data(), (int32_t)ids.size(), 1, E, score.data(), shared.data(), first.data(), &n),
              "LoopDetector::obtainCandidates");
        double minScore = std::numeric_limits<double>::max();
        for (int32_t e = 0; e < E; e++) {
            Frame* k = entries_[e].get();
            fid[e] = k->id();
            if (k == pKF.get()) skip[e] = 1;
            if (k == pKF.get() || !conn.count(k)) continue;
            skip[e] = 1;
            if (rev[e] < minScore) minScore = rev[e];
        }
        int32_t pick[5], np = 0;
        if (rgbd_loop_candidates(E, score.data(), shared.data(), first.data(), fid.data(), skip.data(), pKF->id(), minScore, mnInterval,
                                 pick, &np) != RGBD_OK)
            throw Error("LoopDetector::obtainCandidates: bad arguments");
        for (int32_t i = 0; i < np; i++) {
            entries_[pick[i]]->mScore = score[pick[i]];
            out.push_back(entries_[pick[i]]);
        }
        return out;
    }
    void setInterval(int interval) { mnInterval = interval; }

private:
    std::shared_ptr<Vocabulary> voc_;
    int mnInterval;
    std::vector<Frame::Ptr> entries_;
};

class Matcher {
public:
    explicit Matcher(rgbd_ctx* ctx, float nnratio = 0.6f) : ctx_(ctx), mfNNratio(nnratio) {}
    int match(const Frame& ref, const Frame& cur, std::vector<rgbd_dmatch>& vMatches12, bool discardOutliers = true)
    {
        vMatches12.resize(std::max(ref.N, 1));
        int m = 0;
        const std::vector<float> zq = ref.depths(), zt = cur.depths();
        check(ctx_, rgbd_match(ctx_, ref.mDescriptors.data(), ref.N, cur.mDescriptors.data(), cur.N,
                               ref.mvbOutlier.data(), zq.data(), zt.data(), mfNNratio, discardOutliers ? 1 : 0,
                               vMatches12.data(), (int)vMatches12.size(), &m), "match");
        vMatches12.resize(m);
        return m;
    }
    // Matcher::projectionMatch (Features/Matcher.cpp:35-104): F1's valid 3D points projected into F2 with the
    // two frame poses, F2's keypoints within th pixels as candidates, assigned greedily in F1 order.  Like the
    // reference it APPENDS to vMatches12, starts from an empty taken set and returns vMatches12.size().
    int projectionMatch(const Frame& F1, const Frame& F2, std::vector<rgbd_dmatch>& vMatches12, float th = 5.0f)
    {
        const size_t n0 = vMatches12.size();
        vMatches12.resize(n0 + (size_t)std::max(F1.N, 1));
        const rgbd_bounds b{F2.mnMinX, F2.mnMaxX, F2.mnMinY, F2.mnMaxY};
        int m = 0;
        const rgbd_status s = rgbd_projection_match(ctx_, F1.mvKeys3Dc.data(), F1.mDescriptors.data(), F1.mvbOutlier.data(), F1.N,
                                                    F1.getPose().data(), F2.mvKeysUn.data(), F2.mvKeys3Dc.data(),
                                                    F2.mDescriptors.data(), F2.N, F2.getPose().data(), &b, th,
                                                    vMatches12.data() + n0, F1.N, &m);
        if (s != RGBD_OK) vMatches12.resize(n0);
        check(ctx_, s, "projectionMatch");
        vMatches12.resize(n0 + (size_t)m);
        return (int)vMatches12.size();
    }

private:
    rgbd_ctx* ctx_;
    float mfNNratio;
};

// RNG and sticky covariance are process-global in the reference (System/Random.cpp, SolverSE3.cpp:284);
// here they live in a Session object the caller owns and passes to every solver.
struct Session {
    explicit Session(uint32_t seed = 1) { rgbd_rng_seed(&rng, seed); }
    rgbd_rng rng{};
    rgbd_sticky sticky{};
};

class RansacSE3 {
public:
    RansacSE3(rgbd_ctx* ctx, Session& s, int iters = 200, unsigned minInlierTh = 20, float maxMahalanobisDist = 3.0f,
              unsigned sampleSize = 4)
        : ctx_(ctx), s_(s), prm_{iters, minInlierTh, maxMahalanobisDist, sampleSize}
    {
    }
    // x2 = mT21 * x1; on success with updateF2, F2's pose = mT21 * pose(F1) (:119-126)
    bool compute(const Frame& F1, Frame& F2, const std::vector<rgbd_dmatch>& m12, bool updateF2 = true)
    {
        mvInliers.resize(std::max<size_t>(m12.size(), 1));
        int n_in = 0, ok = 0;
        check(ctx_, rgbd_ransac_se3(ctx_, F1.mvKeys3Dc.data(), F1.N, F2.mvKeys3Dc.data(), F2.N, m12.data(),
                                    (int)m12.size(), &prm_, &s_.rng, &s_.sticky, updateF2 ? 1 : 0,
                                    F2.mvbOutlier.data(), mT21.data(), mvInliers.data(), &n_in, &rmse, &ok),
              "RansacSE3");
        mvInliers.resize(n_in);
        if (ok && updateF2) {
            Pose P;
            const Pose& A = mT21;
            const Pose& B = F1.getPose();
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++) {
                    double acc = 0.0;   // cv::Mat CV_32F gemm accumulates in double
                    for (int k = 0; k < 4; k++) acc += (double)A[4 * i + k] * (double)B[4 * k + j];
                    P[4 * i + j] = (float)acc;
                }
            F2.setPose(P);
        }
        return ok != 0;
    }

    float rmse = 1e6f;
    std::vector<rgbd_dmatch> mvInliers;
    Pose mT21 = identity();

private:
    rgbd_ctx* ctx_;
    Session& s_;
    rgbd_ransac_params prm_;
};

inline Pose pose_mul(const Pose& A, const Pose& B)   // cv::Mat CV_32F gemm: double accumulation
{
    Pose P;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double acc = 0.0;
            for (int k = 0; k < 4; k++) acc += (double)A[4 * i + k] * (double)B[4 * k + j];
            P[4 * i + j] = (float)acc;
        }
    return P;
}

// Gicp(F1, F2, matches, guess): clouds = F1 / F2 3D of the matches (createCloudsFromMatches); on
// success F2's pose = mT * pose(F1) (Solver/Gicp.cpp:21-35).  Ctor defaults: 15 iterations, 0.08 m.
class Gicp {
public:
    Gicp(rgbd_ctx* ctx, const Frame& F1, Frame& F2, const std::vector<rgbd_dmatch>& matches, const Pose& guess)
        : ctx_(ctx), F1_(F1), F2_(F2), matches_(matches), guess_(guess)
    {
    }
    void setMaximumIterations(int iters) { prm_.max_iterations = iters; }
    void setMaxCorrespondenceDistance(double dist) { prm_.max_corr_dist = dist; }
    void setTransformationEpsilon(double eps) { prm_.transformation_epsilon = eps; }
    bool compute(std::vector<rgbd_dmatch>& /*inliers*/)
    {
        const int M = (int)matches_.size();
        std::vector<float> src((size_t)std::max(M, 1) * 3), tgt((size_t)std::max(M, 1) * 3);
        for (int i = 0; i < M; i++)
            for (int k = 0; k < 3; k++) {
                src[3 * i + k] = F1_.mvKeys3Dc[3 * (size_t)matches_[i].queryIdx + k];
                tgt[3 * i + k] = F2_.mvKeys3Dc[3 * (size_t)matches_[i].trainIdx + k];
            }
        int ok = 0;
        check(ctx_, rgbd_gicp_compute(ctx_, src.data(), tgt.data(), M, guess_.data(), &prm_, mT.data(), &ok), "Gicp");
        if (ok && mbUpdate) F2_.setPose(pose_mul(mT, F1_.getPose()));
        return ok != 0;
    }

    bool mbUpdate = true;
    Pose mT = identity();

private:
    rgbd_ctx* ctx_;
    const Frame& F1_;
    Frame& F2_;
    const std::vector<rgbd_dmatch>& matches_;
    Pose guess_;
    rgbd_gicp_params prm_{15, 20, 0.08, 1e-9, 2e-3, 1e-3, 4, 1};
};

// PnPRansac(F1, F2, matches).compute(inliers) (Solver/PnPRansac.cpp:14-56).  as_written = true keeps
// the reference's code as it stands: object points = F2's own back-projection (unprojectWorld with F2's
// current pose, :28-30), and the pose Converter::toHomogeneous builds (:42, System/Converter.cpp:27-37):
// Rodrigues reallocates R as CV_64F, and R.copyTo(Tcw.rowRange(0, 3).colRange(0, 3)) hands a temporary ROI
// to an _OutputArray(const Mat&), which is FIXED_TYPE | FIXED_SIZE; Mat::copyTo into a fixed-type
// destination of another type converts in place (convertTo), so Tcw = [float(R) | float(t)] written into
// Tcw's own data (OpenCV 3.x semantics recalled, parity unpinned: OpenCV is absent) and
// F2's pose becomes that matrix -- not composed with F1's pose.  The default (as_written = false) pairs
// F1's 3D with F2's pixels -- the pairing the tracking benchmark needs -- and sets F2's pose =
// [R|t] pose(F1).  R and t (the solver's rvec / tvec as a rotation matrix) are kept in both modes.
class PnPRansac {
public:
    PnPRansac(rgbd_ctx* ctx, const Frame& F1, Frame& F2, const std::vector<rgbd_dmatch>& matches, bool as_written = false)
        : ctx_(ctx), F1_(F1), F2_(F2), matches_(matches), as_written_(as_written)
    {
    }
    bool compute(std::vector<rgbd_dmatch>& inliers)
    {
        const int M = (int)matches_.size();
        if (M < 10) return false;
        std::vector<float> p3((size_t)M * 3), p2((size_t)M * 2);
        const Pose& Tw = F2_.getPose();   // unprojectWorld: Rwc x + Ow, Twc = Tcw^-1
        for (int i = 0; i < M; i++) {
            const rgbd_dmatch& m = matches_[i];
            const rgbd_keypoint& ku = F2_.mvKeysUn[m.trainIdx];
            p2[2 * i] = ku.x;
            p2[2 * i + 1] = ku.y;
            if (as_written_) {
                // Frame::unprojectWorld (Core/Frame.cpp:317-327): mRwc * x + mOw with the float members
                // set by updatePoseMatrices (:143-153): Rwc = Rcw^T, Ow = -Rcw^T tcw (cv::Mat gemm,
                // double accumulation, one rounding; alpha = -1 for Ow, + Ow as the gemm's C term)
                const float* x = &F2_.mvKeys3Dc[3 * (size_t)m.trainIdx];
                for (int r = 0; r < 3; r++) {
                    double o = 0.0;
                    for (int k = 0; k < 3; k++) o += (double)Tw[4 * k + r] * (double)Tw[4 * k + 3];
                    const float Ow = (float)(o * -1.0);
                    double a = 0.0;
                    for (int k = 0; k < 3; k++) a += (double)Tw[4 * k + r] * (double)x[k];
                    p3[3 * i + r] = (float)(a * 1.0 + (double)Ow * 1.0);
                }
            } else {
                for (int r = 0; r < 3; r++) p3[3 * i + r] = F1_.mvKeys3Dc[3 * (size_t)m.queryIdx + r];
            }
            F2_.mvbOutlier[m.trainIdx] = 1;
        }
        const float K4[4] = {F2_.mCamera.fx, F2_.mCamera.fy, F2_.mCamera.cx, F2_.mCamera.cy};   // mpCamera->k()
        rgbd_pnp_params prm{500, 3.0f, 0.85, 10, 0};
        std::vector<uint8_t> mask(M);
        int ninl = 0, iters = 0, ok = 0;
        check(ctx_, rgbd_pnp_ransac(ctx_, p3.data(), p2.data(), M, K4, &prm, R.data(), t.data(), mask.data(), &ninl,
                                    &iters, &ok), "PnPRansac");
        if (!ok) return false;
        Pose T = identity();
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
            T[4 * r + 3] = (float)t[r];
        }
        F2_.setPose(as_written_ ? T : pose_mul(T, F1_.getPose()));   // as written: toHomogeneous's [float(R) | float(t)]
        inliers.clear();
        for (int i = 0; i < M; i++)
            if (mask[i]) {
                inliers.push_back(matches_[i]);
                F2_.mvbOutlier[matches_[i].trainIdx] = 0;
            }
        return true;
    }

    std::array<double, 9> R{};
    std::array<double, 3> t{};

private:
    rgbd_ctx* ctx_;
    const Frame& F1_;
    Frame& F2_;
    const std::vector<rgbd_dmatch>& matches_;
    bool as_written_;
};

// PnPSolver(F1, F2, matches).compute(inliers) (Solver/PnPSolver.cpp:31-150): motion-only bundle adjustment of
// F2's pose from its current pose and the matches (rgbd_pnp_solver; DESIGN.md "Motion-only BA definition").
// as_written = true keeps the reference's edges: Xw = F2's own unprojectWorld(trainIdx) under F2's current pose
// (:65); the default pairs F1's unprojectWorld(queryIdx) under F1's pose with F2's pixels.  Every matched train
// index is set inlier first (:68); after the solve F2's flags follow the outlier mask, F2's pose is the refined
// one, and the inliers come back in ascending trainIdx order (the std::map iteration of :141-147), not in match
// order.  Fewer than 3 matches: false, and the pose is left alone.
// Precondition: the train indices are unique (Matcher::match and projectionMatch guarantee it) and the 3D points
// used have z > 0.
class PnPSolver {
public:
    PnPSolver(rgbd_ctx* ctx, const Frame& F1, Frame& F2, const std::vector<rgbd_dmatch>& matches, bool as_written = false)
        : ctx_(ctx), F1_(F1), F2_(F2), matches_(matches), as_written_(as_written)
    {
    }
    // Frame::unprojectWorld (Core/Frame.cpp:317-327) with updatePoseMatrices' float members: cv::Mat gemm, double
    // accumulation, one rounding
    static void unprojectWorld(const Pose& Tw, const float* x, float* xw)
    {
        for (int r = 0; r < 3; r++) {
            double o = 0.0, a = 0.0;
            for (int k = 0; k < 3; k++) {
                o += (double)Tw[4 * k + r] * (double)Tw[4 * k + 3];
                a += (double)Tw[4 * k + r] * (double)x[k];
            }
            const float Ow = (float)(o * -1.0);
            xw[r] = (float)(a * 1.0 + (double)Ow * 1.0);
        }
    }
    bool compute(std::vector<rgbd_dmatch>& inliers)
    {
        const int M = (int)matches_.size();
        std::vector<float> Xw((size_t)std::max(M, 1) * 3), obs((size_t)std::max(M, 1) * 2);
        for (int i = 0; i < M; i++) {
            const rgbd_dmatch& m = matches_[i];
            if (as_written_) unprojectWorld(F2_.getPose(), &F2_.mvKeys3Dc[3 * (size_t)m.trainIdx], &Xw[3 * (size_t)i]);
            else unprojectWorld(F1_.getPose(), &F1_.mvKeys3Dc[3 * (size_t)m.queryIdx], &Xw[3 * (size_t)i]);
            obs[2 * (size_t)i] = F2_.mvKeysUn[m.trainIdx].x;
            obs[2 * (size_t)i + 1] = F2_.mvKeysUn[m.trainIdx].y;
            F2_.mvbOutlier[m.trainIdx] = 0;
        }
        const float K4[4] = {F2_.mCamera.fx, F2_.mCamera.fy, F2_.mCamera.cx, F2_.mCamera.cy};
        std::vector<uint8_t> mask((size_t)std::max(M, 1));
        Pose T = identity();
        int ninl = 0, ok = 0;
        check(ctx_, rgbd_pnp_solver(ctx_, Xw.data(), obs.data(), M, K4, F2_.getPose().data(), nullptr, T.data(), mask.data(),
                                    &ninl, &ok), "PnPSolver");
        if (!ok) return false;
        std::map<int, std::pair<rgbd_dmatch, bool>> matchesFlag;
        for (int i = 0; i < M; i++) {
            F2_.mvbOutlier[matches_[i].trainIdx] = mask[i];
            matchesFlag[matches_[i].trainIdx] = {matches_[i], mask[i] == 0};
        }
        F2_.setPose(T);
        inliers.clear();
        for (const auto& kv : matchesFlag)
            if (kv.second.second) inliers.push_back(kv.second.first);
        return true;
    }

private:
    rgbd_ctx* ctx_;
    const Frame& F1_;
    Frame& F2_;
    const std::vector<rgbd_dmatch>& matches_;
    bool as_written_;
};

// Ransac(F1, F2, matches, parameters).compute(inliers) (Solver/Ransac.cpp:12-59): the plain 3D-3D RANSAC on Umeyama
// fits (rgbd_ransac_umeyama; DESIGN.md "Umeyama RANSAC definition").  The context and the Session (the process-global
// rand() of the reference) come first, as with the other solvers here.  compute flags every matched train index of
// F2 outlier and the final inliers' inlier, always sets F2's pose = inv(T) * pose(F1) (:53), and returns
// !T.isIdentity(): a static camera returns false with its inliers set.  iterationCount is ignored, as in the
// reference (:26); the reprojection and Mahalanobis versions throw (RGBD_ERR_UNSUPPORTED).
class Ransac {
public:
    enum ERROR_VERSION { EUCLIDEAN_ERROR, REPROJECTION_ERROR, EUCLIDEAN_AND_REPROJECTION_ERROR, MAHALANOBIS_ERROR, ADAPTIVE_ERROR };
    struct parameters {
        int verbose;
        int errorVersion, errorVersionVO, errorVersionMap;
        double inlierThresholdEuclidean, inlierThresholdReprojection, inlierThresholdMahalanobis;
        double minimalInlierRatioThreshold;
        int minimalNumberOfMatches;
        int usedPairs;
        int iterationCount;
    };
    Ransac(rgbd_ctx* ctx, Session& s, const Frame& F1, Frame& F2, const std::vector<rgbd_dmatch>& matches, parameters params)
        : ctx_(ctx), s_(s), F1_(F1), F2_(F2), matches_(matches),
          prm_{params.errorVersion, params.usedPairs, params.minimalNumberOfMatches, 0, params.inlierThresholdEuclidean,
               params.minimalInlierRatioThreshold}
    {
    }
    bool compute(std::vector<rgbd_dmatch>& inliers)
    {
        const int M = (int)matches_.size();
        inliers.resize((size_t)std::max(M, 1));
        int n_in = 0, ok = 0;
        check(ctx_, rgbd_ransac_umeyama(ctx_, F1_.mvKeys3Dc.data(), F1_.N, F2_.mvKeys3Dc.data(), F2_.N, matches_.data(), M, &prm_,
                                        &s_.rng, F2_.mvbOutlier.data(), mT12.data(), inliers.data(), &n_in, &iterations, &ok),
              "Ransac");
        inliers.resize((size_t)n_in);
        Pose P;
        rgbd_ransac_umeyama_pose(mT12.data(), F1_.getPose().data(), P.data());
        F2_.setPose(P);
        return ok != 0;
    }

    Pose mT12 = identity();   // x1 = mT12 * x2: F2's camera points in F1's camera
    int iterations = 0;       // RANSAC iterations run

private:
    rgbd_ctx* ctx_;
    Session& s_;
    const Frame& F1_;
    Frame& F2_;
    const std::vector<rgbd_dmatch>& matches_;
    rgbd_umeyama_params prm_;
};

}  // namespace rgbd
