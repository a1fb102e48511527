// The mutable half of a key (bzh_pk and bzh_vk each hold ONE KeyRuntime): the key's mutex, the per-call device workspaces and the
// count of calls running on the key.  Host code only; depends on the HIP runtime header (the arena's allocations).  Included
// inside namespace bzh { namespace { by csrc/key_shape.hpp; tests/helpers/key_runtime_check.hip drives it without a device.
#pragma once

// device arena: grow-only blocks, reset at the start of every call
struct Arena {
    struct Block {
        char* p;
        size_t size, used;
    };
    std::vector<Block> blocks;
    int device = 0;
    size_t live = 0, peak = 0;  // bytes handed out and not released since the last reset, and their high-water mark
    // A call's allocation sequence is deterministic, so after the first call of a given shape the arena is ONE block
    // that every later call bumps through without touching hipMalloc (overflow blocks are merged at the next reset).
    void reset() {
        if (blocks.size() > 1) {
            const size_t want = peak + (peak >> 4) + ((size_t)1 << 20);
            release();
            Block nb;
            nb.size = want;
            nb.used = 0;
            if (hipMalloc((void**)&nb.p, nb.size) == hipSuccess) blocks.push_back(nb);
        }
        for (auto& b : blocks) b.used = 0;
        live = peak = 0;
    }
    void release() {
        for (auto& b : blocks) (void)hipFree(b.p);
        blocks.clear();
    }
    // device bytes the arena holds right now (bzh_pk_device_bytes / bzh_vk_device_bytes)
    size_t held() const {
        size_t s = 0;
        for (auto& b : blocks) s += b.size;
        return s;
    }
    void* alloc(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        live += bytes;
        peak = std::max(peak, live);
        for (auto& b : blocks)
            if (b.size - b.used >= bytes) {
                void* r = b.p + b.used;
                b.used += bytes;
                return r;
            }
        Block nb;
        nb.size = std::max(bytes, (size_t)256 << 20);
        if (hipMalloc((void**)&nb.p, nb.size) != hipSuccess) return nullptr;
        nb.used = bytes;
        blocks.push_back(nb);
        return nb.p;
    }
    // Stack discipline for temporaries (a commitment's scalar vectors, gathered rows): everything allocated after mark() is
    // handed back by pop().  Work on the buffers was enqueued on the ctx's one stream, so whatever reuses the memory runs
    // after it.  While the arena is still a list of blocks (a key's first call) only the accounting moves: the merged block
    // of the next call is sized by the high-water mark.
    struct Mark {
        size_t used, live;
        bool single;
    };
    Mark mark() const { return Mark{blocks.size() == 1 ? blocks[0].used : 0, live, blocks.size() == 1}; }
    void pop(const Mark& m) {
        live = m.live;
        if (m.single && blocks.size() == 1) blocks[0].used = m.used;
    }
};
struct ArenaScope {
    Arena& a;
    Arena::Mark m;
    explicit ArenaScope(Arena& ar) : a(ar), m(ar.mark()) {}
    ~ArenaScope() { a.pop(m); }
};

// A key is immutable after its creation except for caches filled on first use and what is kept here.  Calls through different
// ctxs run concurrently on one key; a call holds its ctx's mutex throughout (lock order: ctx->mu, then the key's `mu`), and `mu`
// is only ever held for short sections.
struct KeyRuntime {
    std::mutex mu;
    // Per-call workspaces: one grow-only arena per ctx SERIAL (bzh_ctx::serial) that has used the key, so that several worker
    // streams share ONE key.  A serial is never handed out twice: the arena of a destroyed ctx stays until the key is freed, and
    // no later ctx -- whatever its address or device -- can pick it up.
    std::map<uint64_t, std::unique_ptr<Arena>> arenas;
    // Calls running on the key right now, over all ctxs, counted from their first line (Call, below): what unloads the key's
    // code or frees its arenas refuses while this is non-zero.  Guarded by `mu`.
    int calls = 0;

    Arena& arena_for(uint64_t ctx_serial, int device) {
        std::lock_guard<std::mutex> lk(mu);
        auto& a = arenas[ctx_serial];
        if (!a) {
            a.reset(new Arena());
            a->device = device;
        }
        return *a;
    }
    // device bytes held over all arenas (the caller holds `mu`)
    size_t held_locked() const {
        size_t s = 0;
        for (auto& kv : arenas) s += kv.second->held();
        return s;
    }
    // One call on the key, from its entry into the library to its return.  Takes `mu` for the increment and the decrement only,
    // and is constructed and destroyed outside every other lock, so it never nests.
    struct Call {
        KeyRuntime& rt;
        explicit Call(KeyRuntime& r) : rt(r) {
            std::lock_guard<std::mutex> lk(rt.mu);
            rt.calls++;
        }
        ~Call() {
            std::lock_guard<std::mutex> lk(rt.mu);
            rt.calls--;
        }
        Call(const Call&) = delete;
    };
    // The key is about to be freed.  Under `mu`: false, nothing touched, while a call is running; otherwise every device that
    // holds a non-empty arena is synchronised (the arenas belong to the streams of all ctxs) and every arena is released.  After
    // `true` the owner deletes the key; a call that starts later is the caller's error (include/bzh2.h).
    bool retire() {
        std::lock_guard<std::mutex> lk(mu);
        if (calls) return false;
        for (auto& kv : arenas) {
            if (kv.second->blocks.empty()) continue;
            (void)hipSetDevice(kv.second->device);
            (void)hipDeviceSynchronize();
            kv.second->release();
        }
        arenas.clear();
        return true;
    }
};
