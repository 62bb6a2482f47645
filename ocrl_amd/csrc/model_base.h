// What the stateful models (SLATE, IODINE) share behind the C ABI: the published parameter table over one flat fp32 buffer, the
// caller-allocated workspace carved into (optionally named) tensors, and the lookup of both by name.  The layout policy lives
// here and nowhere else: parameter offsets are 16-byte aligned, workspace tensors 256-byte aligned, the sizing pass is the layout
// pass run on a null base pointer, and a name resolves to a workspace tensor first, then to a parameter.
#pragma once
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "common.h"

struct ParamInfo {
    std::string name;
    int shape[4] = {1, 1, 1, 1};
    int ndim = 1;
    long long numel = 0;
    long long offset = 0;   // element offset into the flat parameter buffer (16-byte aligned)
    int group = 0;          // optimiser group (SLATE: 0 dvae, 1 slot-attention side, 2 transformer decoder; IODINE has one)
};

// A parameter resolved by name once, when the model is created: its element offset into the flat buffers.  An offset, not a pointer:
// bind() may be called again with other buffers.  ModelBase::P / G turn it into the parameter / gradient pointer of the current binding.
struct ParamRef { long long off = 0; };
struct ParamPair { ParamRef w, b; };       // "<prefix>.weight" and "<prefix>.bias" of one layer

class ModelBase {
public:
    ModelBase(const ModelBase&) = delete;
    ModelBase& operator=(const ModelBase&) = delete;
    const std::vector<ParamInfo>& params() const { return params_; }
    long long flat_size() const { return flat_size_; }
    size_t workspace_bytes() const { return ws_bytes_; }
    float* metrics() const { return metrics_; }                 // device float[8], carved by the model's layout
    // empty, or what made the constructor's resolve fail (the first name that is not in the parameter table): the create entry point
    // reports it and discards the model
    const std::string& create_error() const { return create_error_; }
    int tensor(const char* name, float** ptr, long long* count) const {
        auto it = named_.find(name);
        if (it == named_.end()) {
            auto pi = index_.find(name);
            OCRL_REQUIRE(pi != index_.end(), "tensor: unknown name '%s'", name);
            *ptr = p_ + params_[pi->second].offset;
            *count = params_[pi->second].numel;
            return 0;
        }
        *ptr = it->second.first;
        *count = (long long)it->second.second;
        return 0;
    }

protected:
    ModelBase() = default;
    ~ModelBase() = default;

    // ---- parameter table: add_param() in the reference module's parameters() order, then finish_params() once
    void add_param(const std::string& name, const std::vector<int>& shp, int group = 0) {
        ParamInfo p;
        p.name = name; p.ndim = (int)shp.size(); p.group = group; p.numel = 1;
        for (size_t i = 0; i < shp.size(); ++i) { p.shape[i] = shp[i]; p.numel *= shp[i]; }
        params_.push_back(p);
    }
    static long long padded(long long numel) { return (numel + 3) & ~3ll; }       // keep every tensor 16-byte aligned (float4 / MFMA staging)
    // with `groups` > 0 (parameters added in group order): group g = [group_begin[g], group_begin[g + 1]), groups + 1 entries
    void finish_params(long long* group_begin = nullptr, int groups = 0) {
        long long off = 0;
        int g = 0;
        if (groups) group_begin[0] = 0;
        for (size_t i = 0; i < params_.size(); ++i) {
            while (g < groups && g < params_[i].group) group_begin[++g] = off;
            params_[i].offset = off;
            off += padded(params_[i].numel);
            index_[params_[i].name] = (int)i;
        }
        while (g < groups) group_begin[++g] = off;
        flat_size_ = off;
    }
    // by-name lookup for the constructors only (after finish_params()): the step path holds ParamRefs, so a misspelt name fails the
    // create call whatever branch would have used it, and no launch builds a string or searches the index
    ParamRef ref(const std::string& n) {
        auto it = index_.find(n);
        if (it != index_.end()) return ParamRef{params_[it->second].offset};
        if (create_error_.empty()) create_error_ = "unknown parameter '" + n + "'";
        return ParamRef();
    }
    ParamPair ref_pair(const std::string& prefix) { return ParamPair{ref(prefix + ".weight"), ref(prefix + ".bias")}; }
    float* P(ParamRef r) const { return p_ + r.off; }
    float* G(ParamRef r) const { return g_ + r.off; }

    // ---- workspace: a layout pass is begin_layout(), the model's carve() calls in a fixed order (the order is the layout),
    // end_layout().  The constructor runs it without a buffer (commit = false) to size the workspace, bind() on the caller's.
    void begin_layout(bool commit) { ws_commit_ = commit; ws_off_ = 0; }
    float* carve_pos() const { return reinterpret_cast<float*>(ws_ + ws_off_); }     // where the next carve() will land
    float* carve(const char* name, size_t n) {
        const size_t bytes = (n * 4 + 255) & ~(size_t)255;
        float* p = carve_pos();
        ws_off_ += bytes;
        if (ws_commit_ && name) named_[name] = std::make_pair(p, n);
        return p;
    }
    void end_layout() { if (!ws_commit_) ws_bytes_ = ws_off_ + 4096; }

    // ---- bind(): check_buffers(), then the model's own configuration checks, then adopt_buffers() -- a rejected call leaves
    // the previous binding in place and the first failing check decides the message
    int check_buffers(const float* p, const float* g, const void* ws, size_t ws_bytes) const {
        OCRL_REQUIRE(p && g && ws, "bind: null buffer");
        OCRL_REQUIRE(ws_bytes >= ws_bytes_, "bind: workspace too small (%zu < %zu)", ws_bytes, ws_bytes_);
        OCRL_REQUIRE(((uintptr_t)p & 255) == 0 && ((uintptr_t)g & 255) == 0 && ((uintptr_t)ws & 255) == 0, "bind: buffers must be 256-byte aligned");
        return 0;
    }
    void adopt_buffers(float* p, float* g, float* m, float* v, void* ws) {
        p_ = p; g_ = g; m_ = m; v_ = v;
        ws_ = static_cast<char*>(ws);
        named_.clear();
    }

    std::vector<ParamInfo> params_;
    std::map<std::string, int> index_;
    long long flat_size_ = 0;
    float *p_ = nullptr, *g_ = nullptr, *m_ = nullptr, *v_ = nullptr;
    char* ws_ = nullptr;
    size_t ws_bytes_ = 0, ws_off_ = 0;
    bool ws_commit_ = false;
    std::map<std::string, std::pair<float*, size_t>> named_;
    float* metrics_ = nullptr;
    std::string create_error_;
};
