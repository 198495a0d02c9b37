// The kernel timers' deferred event pairs (rcorrector_amd/csrc/rc_timer_pool.h) against a stub back end whose "streams" are
// clocks: record() stamps an event with its stream's time, wait() marks it waited for, elapsed() refuses an end event nobody
// waited for since it was last recorded (what the library must never ask of HIP).  Prints "ok <checks>".
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rc_timer_pool.h"

static int g_checks = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        ++g_checks;                                                \
        if (!(c)) {                                                \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            exit(1);                                               \
        }                                                          \
    } while (0)

struct stub_event {
    double at = 0;
    bool recorded = false, waited = false;
};

struct stub_events {
    typedef stub_event *event;
    typedef double *stream;  // a stream is its clock, in ms
    int created = 0, destroyed = 0, waits = 0, unwaited_reads = 0, fail_create_after = -1;
    bool create(event *e)
    {
        if (fail_create_after >= 0 && created >= fail_create_after) return false;
        *e = new stub_event();
        ++created;
        return true;
    }
    void destroy(event e)
    {
        delete e;
        ++destroyed;
    }
    void record(event e, stream st)
    {
        e->at = *st;
        e->recorded = true;
        e->waited = false;
    }
    void wait(event e)
    {
        e->waited = true;
        ++waits;
    }
    bool elapsed(event a, event b, float *ms)
    {
        if (!a->recorded || !b->recorded) return false;
        if (!b->waited) ++unwaited_reads;
        *ms = (float)(b->at - a->at);
        return true;
    }
};

enum { KINDS = 4, CAP = 6 };
typedef rc_timer_pool<stub_events, KINDS, CAP> pool_t;

int main()
{
    double s1 = 0, s2 = 100;  // two streams
    {   // one pair, resolved twice: counted once
        pool_t p;
        const int a = p.begin(&s1);
        CHECK(a >= 0);
        s1 += 5;
        p.end(a, 2, &s1);
        CHECK(p.total[2].launches == 0 && p.be.waits == 0);  // (nothing waits before resolve)
        p.resolve();
        CHECK(p.total[2].launches == 1 && p.total[2].ms == 5.0 && p.be.waits == 1);
        p.resolve();
        CHECK(p.total[2].launches == 1 && p.total[2].ms == 5.0 && p.be.waits == 1);
        CHECK(p.be.unwaited_reads == 0);
        p.release();
        CHECK(p.be.created == 2 && p.be.destroyed == 2);
    }
    {   // pairs of several kinds open at once on two streams (the pipeline: one per kernel kind), closed out of order
        pool_t p;
        const int probe = p.begin(&s1), single = p.begin(&s2), correct = p.begin(&s2);
        CHECK(probe >= 0 && single >= 0 && correct >= 0 && probe != single && single != correct && probe != correct);
        s1 += 30;
        s2 += 7;
        p.end(single, 3, &s2);
        p.end(probe, 0, &s1);
        p.resolve();  // (the pair that is still open stays open)
        CHECK(p.total[3].ms == 7.0 && p.total[0].ms == 30.0 && p.total[2].launches == 0);
        s2 += 11;
        p.end(correct, 2, &s2);
        p.end(correct, 2, &s2);  // (ended twice: the second is ignored)
        p.resolve();
        CHECK(p.total[2].ms == 18.0 && p.total[2].launches == 1);
        p.end(-1, 0, &s1);       // (no pair: ignored)
        p.end(CAP, 0, &s1);
        p.end(probe, 0, &s1);    // (a pair that is free again: ignored)
        p.end(single, KINDS, &s2);
        p.resolve();
        CHECK(p.total[0].launches == 1 && p.total[3].launches == 1 && p.be.unwaited_reads == 0);
        p.release();
    }
    {   // pool full: begin() resolves the closed pairs and goes on; events are reused, never created twice
        pool_t p;
        for (int round = 0; round < 5; ++round)
            for (int i = 0; i < CAP; ++i) {
                const int a = p.begin(&s1);
                CHECK(a >= 0);
                s1 += 1;
                p.end(a, i % KINDS, &s1);
            }
        p.resolve();
        uint64_t n = 0;
        double ms = 0;
        for (int kd = 0; kd < KINDS; ++kd) {
            n += p.total[kd].launches;
            ms += p.total[kd].ms;
        }
        CHECK(n == 5 * CAP && ms == 5.0 * CAP && p.be.created == 2 * CAP && p.be.unwaited_reads == 0);
        // every pair open: no pair to hand out, and nothing breaks; the open pairs can still be ended
        int open[CAP];
        for (int i = 0; i < CAP; ++i) CHECK((open[i] = p.begin(&s1)) >= 0);
        CHECK(p.begin(&s1) == -1);
        p.end(-1, 0, &s1);
        s1 += 2;
        for (int i = 0; i < CAP; ++i) p.end(open[i], 1, &s1);
        CHECK(p.begin(&s1) >= 0);  // (full of closed pairs: resolved on the way)
        CHECK(p.total[1].launches == 10 + CAP);  // (kinds 0 1 2 3 0 1 in each of the five rounds, then the six)
        p.release();
        CHECK(p.be.created == p.be.destroyed);
    }
    {   // reset while pairs are pending: they are dropped unmeasured, the sums are zero, the pool is whole again
        pool_t p;
        const int a = p.begin(&s1), b = p.begin(&s2), c = p.begin(&s1);
        s1 += 3;
        p.end(a, 0, &s1);
        p.end(c, 1, &s1);
        p.resolve();
        const int d = p.begin(&s1);
        s1 += 4;
        p.end(d, 0, &s1);  // closed, pending; b is open, pending
        p.reset();
        for (int kd = 0; kd < KINDS; ++kd) CHECK(p.total[kd].launches == 0 && p.total[kd].ms == 0);
        p.resolve();
        for (int kd = 0; kd < KINDS; ++kd) CHECK(p.total[kd].launches == 0 && p.total[kd].ms == 0);
        p.end(b, 2, &s2);  // (the end of a pair the reset dropped: ignored)
        p.resolve();
        CHECK(p.total[2].launches == 0);
        for (int i = 0; i < CAP; ++i) {  // all of the pool is free again, on the events it had
            const int e = p.begin(&s2);
            CHECK(e >= 0);
            s2 += 1;
            p.end(e, 3, &s2);
        }
        p.resolve();
        CHECK(p.total[3].launches == CAP && p.total[3].ms == (double)CAP && p.be.unwaited_reads == 0);
        // a launcher that starts its timer twice: the later begin counts
        const int f = p.begin(&s1);
        s1 += 9;
        p.rebegin(f, &s1);
        s1 += 1;
        p.end(f, 0, &s1);
        p.resolve();
        CHECK(p.total[0].launches == 1 && p.total[0].ms == 1.0);
        p.release();
        p.release();  // (twice: nothing is destroyed twice)
        CHECK(p.be.created == p.be.destroyed);
    }
    {   // an event cannot be created: the interval is not measured, nothing leaks
        pool_t p;
        p.be.fail_create_after = 1;
        CHECK(p.begin(&s1) == -1);
        CHECK(p.be.created == 1 && p.be.destroyed == 1);
        p.be.fail_create_after = -1;
        const int a = p.begin(&s1);
        CHECK(a >= 0);
        p.end(a, 0, &s1);
        p.resolve();
        CHECK(p.total[0].launches == 1);
        p.release();
        CHECK(p.be.created == p.be.destroyed);
    }
    printf("ok %d checks\n", g_checks);
    return 0;
}
