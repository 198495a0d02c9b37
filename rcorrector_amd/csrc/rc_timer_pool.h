// rc_timer_pool.h -- the kernel timers' deferred event pairs.  Plain host code over an event back end `B`, so that
// tests/hostmath/timer_pool.cpp can drive it against a stub; the library's back end is HIP's events (rc_api.hip).
//
// A timer used to be two events and a hipEventSynchronize behind every kernel: with profiling on (bench.py's timed steps) the
// host then waited for each kernel before it queued the next, and two streams could never run side by side.  Now begin() /
// end() only RECORD a pair of events on a stream, and resolve() -- rc_profile_get, rc_sync, or begin() on a full pool -- waits
// for the pairs' end events and adds their elapsed times up.  A pair counts one launch, whatever was queued between its two
// events (the chunked pipeline puts one pair around all the chunks' kernels of a kind).
//
// B provides:  typedef event, typedef stream;
//              bool create(event *);  void destroy(event);  void record(event, stream);  void wait(event);
//              bool elapsed(event begin, event end, float *ms);
#pragma once
#include <stdint.h>

template <class B, int KINDS, int CAP = 32>
struct rc_timer_pool {
    struct acc {
        double ms = 0;
        uint64_t launches = 0;
    };
    enum : uint8_t { FREE = 0, OPEN = 1, CLOSED = 2 };  // OPEN: begin recorded; CLOSED: end recorded too, not added up yet
    struct pair {
        typename B::event e0, e1;
        uint8_t state = FREE;
        bool made = false;
        int kind = 0;
    };
    B be;
    pair pairs[CAP];
    acc total[KINDS];
    int n_closed = 0;

    // a pair whose begin event is recorded on `st`; -1: no event could be created (the interval is not measured).  A full pool
    // resolves itself first; pairs that are open then (their end is still to come) stay, and if every pair is open, -1.
    int begin(typename B::stream st)
    {
        int at = find_free();
        if (at < 0) {
            resolve();
            at = find_free();
        }
        if (at < 0) return -1;
        pair &p = pairs[at];
        if (!p.made) {
            if (!be.create(&p.e0)) return -1;
            if (!be.create(&p.e1)) {
                be.destroy(p.e0);
                return -1;
            }
            p.made = true;
        }
        be.record(p.e0, st);
        p.state = OPEN;
        return at;
    }
    // the begin event of an open pair once more (a launcher that starts its timer twice)
    void rebegin(int at, typename B::stream st)
    {
        if (at >= 0 && at < CAP && pairs[at].state == OPEN) be.record(pairs[at].e0, st);
    }
    void end(int at, int kind, typename B::stream st)
    {
        if (at < 0 || at >= CAP || pairs[at].state != OPEN || kind < 0 || kind >= KINDS) return;
        be.record(pairs[at].e1, st);
        pairs[at].kind = kind;
        pairs[at].state = CLOSED;
        ++n_closed;
    }
    // waits for every closed pair and adds it to its kind; open pairs stay open.  Nothing closed: nothing happens
    void resolve()
    {
        if (!n_closed) return;
        for (pair &p : pairs) {
            if (p.state != CLOSED) continue;
            be.wait(p.e1);
            float ms = 0;
            if (be.elapsed(p.e0, p.e1, &ms)) {
                total[p.kind].ms += ms;
                total[p.kind].launches += 1;
            }
            p.state = FREE;
        }
        n_closed = 0;
    }
    // the sums to zero; pairs that are pending -- closed or open -- are dropped unmeasured (their events may still be in a
    // stream: they are kept and recorded anew by their next use, which is what HIP allows of an event)
    void reset()
    {
        for (pair &p : pairs) p.state = FREE;
        n_closed = 0;
        for (acc &a : total) a = acc();
    }
    void release()
    {
        for (pair &p : pairs) {
            if (p.made) {
                be.destroy(p.e0);
                be.destroy(p.e1);
            }
            p.made = false;
            p.state = FREE;
        }
        n_closed = 0;
    }

private:
    int find_free() const
    {
        for (int i = 0; i < CAP; ++i)
            if (pairs[i].state == FREE) return i;
        return -1;
    }
};
