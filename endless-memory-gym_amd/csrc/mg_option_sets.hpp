// mg_option_sets.hpp -- per-instance option sets of one handle (include/memgym.h: mg_set_option_set / mg_bind_option_sets).
//
// A family supplies `Opt`: its parameter block `P` (what the kernels read) next to the OptListStores and raw option values that
// stand behind it, and `static void copy_geometry(Params& dst, const Params& src)`, the fields the handle's shared atlases,
// tables and launch arrangement fix for every set.  Set 0 is the handle-wide set of mg_set_option and always exists; sets > 0
// hold everything that does not change the geometry and take set 0's.
#pragma once
#include <memory>
#include <vector>

#include "mg_family.hpp"

namespace mg {

template <typename Opt>
class OptionSets {
   public:
    using Params = decltype(Opt::P);
    OptionSets() { opt_.emplace_back(new Opt()); }
    void alloc() { dev_.alloc(MG_MAX_OPTION_SETS); }
    Opt& operator[](size_t set) { return *opt_[set]; }
    size_t size() const { return opt_.size(); }
    // the constructor's defaults (= the reference's): what a new set starts from and what a set that was never written holds.
    // Short lists only: no device arrays behind them.
    Params defaults;

    // Set `set`, created if need be together with the ones below it: the defaults under the handle's geometry (`init`: what
    // the family derives from a set's raw values)
    template <typename Init>
    Opt& ensure(int set, Init init) {
        if (set < 0 || set >= MG_MAX_OPTION_SETS) throw OptionError{-3, "option set index out of range"};
        while ((int)opt_.size() <= set) {
            opt_.emplace_back(new Opt());
            opt_.back()->P = defaults;
            Opt::copy_geometry(opt_.back()->P, opt_[0]->P);
            init(*opt_.back());
        }
        dirty_ = true;
        return *opt_[set];
    }
    Opt& ensure(int set) { return ensure(set, [](Opt&) {}); }

    // instance i runs under option set set_of_dev[i] (device array [num_envs], caller-owned; NULL: every instance under set 0)
    void bind(const int32_t* set_of_dev) { set_of_ = set_of_dev; }
    bool per_set() const { return set_of_ != nullptr && opt_.size() > 1; }
    // what a kernel-argument struct carries: both null unless the instances run under sets of their own
    const Params* dev() const { return per_set() ? dev_.p : nullptr; }
    const int32_t* set_of() const { return per_set() ? set_of_ : nullptr; }

    // set 0's geometry changed (a rebuild, a capacity): every other set and the defaults follow
    void refresh_geometry() {
        for (size_t k = 1; k < opt_.size(); ++k) Opt::copy_geometry(opt_[k]->P, opt_[0]->P);
        Opt::copy_geometry(defaults, opt_[0]->P);
        dirty_ = true;
    }
    void touch() { dirty_ = true; }
    // the sets as the kernels read them, stream-ordered behind what the stream holds (pageable source: staged before the call returns)
    void upload(hipStream_t s) {
        if (!per_set() || !dirty_) return;
        // Geometry once more: set 0 carries fields that change without a rebuild (Searing Spotlights: ordered_holes may have been
        // switched on since; Mystery Path: the launch arrangement's lazy / pre flags, which are 0 whenever sets are in use, so
        // that sets > 0 generate every path segment when it is due)
        refresh_geometry();
        std::vector<Params> host(MG_MAX_OPTION_SETS, defaults);  // (a set that was never written: the defaults, include/memgym.h)
        for (size_t k = 0; k < opt_.size(); ++k) host[k] = opt_[k]->P;
        MG_HIP(hipMemcpyAsync(dev_.p, host.data(), sizeof(Params) * host.size(), hipMemcpyHostToDevice, s));
        MG_HIP(hipStreamSynchronize(s));  // (rare: only after an option of some set changed)
        dirty_ = false;
    }

   private:
    std::vector<std::unique_ptr<Opt>> opt_;  // [0] = the handle-wide set
    const int32_t* set_of_ = nullptr;
    bool dirty_ = true;
    DevArray<Params> dev_;
};

}  // namespace mg
