// How a handful of integers reaches the host without a stream synchronise: a launch queues, behind its last kernel, a copy of
// a small device header into a pinned host slot and records an event; the read waits for THAT EVENT, not for the stream, so
// work queued behind the launch goes on while the host reads, allocates and queues what comes next.
// A small ring of slots per device, created on first use and reused; a slot belongs to the workspace pointer it was launched
// with until its read; the library has no teardown, so the slots (sizeof(T) pinned bytes and an event each) live as long as the
// process.  One mutex guards a ring: it is held while a slot is chosen and its copy + event are queued, and while a read looks
// its slot up and copies the bytes out -- never across the wait for the event.
// One ring per user (marching cubes' counts: mc.hip; the component counts: mesh_components.hip), each a static object there.
#pragma once
#include <mutex>

#include "common.h"

namespace sculpt {

template <class T>
struct ReadbackRing {
    static constexpr int SLOTS = 8, DEVICES = 64;
    struct Slot {
        const void *ws;              // the workspace of the pending launch (key; meaningful while `pending`)
        T *host;                     // pinned; null: the slot has not been created yet
        hipEvent_t ev;               // recorded behind the copy into `host`
        bool pending;                // launched and not read yet
        unsigned long long seq;      // launch number: the oldest pending slot gives way when the ring is full
    };
    const char *name;                // prefix of the error messages ("mc_count")
    int no_launch_rc;                // what a read without a pending launch returns
    std::mutex mu;
    Slot ring[DEVICES][SLOTS];
    unsigned long long seq_counter;

    int device(int *dev) {
        SC_HIP(hipGetDevice(dev));
        SC_REQUIRE(*dev >= 0 && *dev < DEVICES, "%s: device %d is beyond the %d the count slots cover", name, *dev, DEVICES);
        return 0;
    }

    // queue the header's copy and the event for the phase just launched on `st` into `workspace`
    int launch(const void *workspace, const T *hdr_dev, hipStream_t st) {
        int dev = 0;
        if (int rc = device(&dev)) return rc;
        std::lock_guard<std::mutex> lock(mu);
        Slot *r = ring[dev], *slot = nullptr;
        for (int i = 0; i < SLOTS && !slot; ++i)   // a second launch on the same workspace replaces the pending one
            if (r[i].host && r[i].pending && r[i].ws == workspace) slot = &r[i];
        for (int i = 0; i < SLOTS && !slot; ++i)
            if (r[i].host && !r[i].pending) slot = &r[i];
        for (int i = 0; i < SLOTS && !slot; ++i)
            if (!r[i].host) slot = &r[i];
        if (!slot) {   // every slot pending: the oldest launch loses its slot (its read reports that no count is pending)
            slot = &r[0];
            for (int i = 1; i < SLOTS; ++i)
                if (r[i].seq < slot->seq) slot = &r[i];
        }
        if (!slot->host) {   // first use of this slot (the current device is `dev`: the event belongs to it)
            void *p = nullptr;
            SC_HIP(hipHostMalloc(&p, sizeof(T), hipHostMallocDefault));
            hipEvent_t ev;
            if (hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) {
                (void)hipHostFree(p);
                set_error("hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
                return 1;
            }
            slot->host = reinterpret_cast<T *>(p);
            slot->ev = ev;
        }
        slot->pending = false;   // (stays so when one of the two calls below fails)
        SC_HIP(hipMemcpyAsync(slot->host, hdr_dev, sizeof(T), hipMemcpyDeviceToHost, st));
        SC_HIP(hipEventRecord(slot->ev, st));
        slot->ws = workspace;
        slot->seq = ++seq_counter;
        slot->pending = true;
        return 0;
    }

    // wait for the pending launch of `workspace` and take its header; the slot is free afterwards
    int read(const void *workspace, T *out) {
        int dev = 0;
        if (int rc = device(&dev)) return rc;
        Slot *r = ring[dev], *slot = nullptr;
        hipEvent_t ev;
        unsigned long long seq;
        {
            std::lock_guard<std::mutex> lock(mu);
            for (int i = 0; i < SLOTS && !slot; ++i)
                if (r[i].host && r[i].pending && r[i].ws == workspace) slot = &r[i];
            if (!slot) {
                set_error("%s_read: no count launch is pending for workspace %p on device %d (read already, never launched, or "
                          "more than %d counts pending)", name, workspace, dev, SLOTS);
                return no_launch_rc;
            }
            ev = slot->ev;
            seq = slot->seq;
        }
        SC_HIP(hipEventSynchronize(ev));
        std::lock_guard<std::mutex> lock(mu);
        if (!slot->pending || slot->seq != seq) {   // another thread launched or read on this workspace meanwhile
            set_error("%s_read: the pending count of workspace %p was replaced while it was being read", name, workspace);
            return no_launch_rc;
        }
        *out = *slot->host;
        slot->pending = false;
        return 0;
    }
};

}  // namespace sculpt
