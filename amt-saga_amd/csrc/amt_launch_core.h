// Book-keeping around a kernel launch: plain C++17 with no HIP include, so that a stand-alone host program tests it under
// the sanitizers (tests/launch_host_main.cpp).  amt_launch.h puts the runtime calls on top.
#ifndef AMT_LAUNCH_CORE_H
#define AMT_LAUNCH_CORE_H
#include <stdlib.h>
#include <map>
#include <mutex>

// The dynamic-LDS limit already granted per (device index, function address): the limit belongs to the function's copy
// on ONE device.  The mutex stays held across the runtime call, so a caller that finds its key at or above what it
// wants knows that the call which granted it has returned.
class amt_lds_limits {
  public:
    // The limit of fn on device is at least bytes when this returns 0.  set(bytes) performs the runtime call and returns
    // 0 on success: it runs on the first request for a key and on every larger one (grow-only), never for a request at
    // or below the record.  Its failure is returned and leaves the record as it was: the next request tries again.
    template <class Set>
    int request(int device, const void *fn, size_t bytes, Set set) {
        std::lock_guard<std::mutex> hold(mu_);
        const auto key = std::make_pair(device, fn);
        const auto it = granted_.find(key);
        if (it != granted_.end() && bytes <= it->second) return 0;
        const int rc = set(bytes);
        if (rc == 0) granted_[key] = bytes;
        return rc;
    }
  private:
    std::mutex mu_;
    std::map<std::pair<int, const void *>, size_t> granted_;
};

// hop a power of two in [lo, hi]: *shift = log2(hop), true.  Anything else: false, *shift untouched.
static inline bool amt_hop_shift(int hop, int lo, int hi, int *shift) {
    if (hop <= 0 || (hop & (hop - 1)) != 0 || hop < lo || hop > hi) return false;
    *shift = 0;
    while ((1 << *shift) < hop) ++*shift;
    return true;
}

// The two readers of the environment.  A value is an integer when ALL of it is one (strtol's syntax: blanks, a sign,
// decimal digits); unset, empty and trailing text are not.
static inline bool amt_env_integer(const char *text, long *v) {
    char *end = nullptr;
    if (text && *text) *v = strtol(text, &end, 10);
    return end && *end == 0;
}
// A switch: unset -> dflt; an integer zero ("0", "00") -> off; any other value (as "1") -> on.
static inline bool amt_env_switch(const char *name, bool dflt) {
    const char *e = getenv(name);
    long v = 0;
    return e ? !(amt_env_integer(e, &v) && v == 0) : dflt;
}
// A number: the value if it is an integer >= lowest, else dflt (unset, empty, text, too small).
static inline long amt_env_number(const char *name, long dflt, long lowest = 1) {
    long v = 0;
    return amt_env_integer(getenv(name), &v) && v >= lowest ? v : dflt;
}
#endif
