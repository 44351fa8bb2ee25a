// vmorph/worker.hpp -- what the facade's thread classes (MatchingThread, VideoMatchingThread, SyncThread; the
// reference's QThread subclasses) share: the cancel flag, run_time, and a std::thread whose exception
// reaches the caller of wait().  Standard headers only.
#ifndef VMORPH_WORKER_HPP
#define VMORPH_WORKER_HPP

#include <chrono>
#include <exception>
#include <thread>

namespace vmorph {
namespace detail {

class Worker {
public:
    Worker() : runflag(1) {}
    Worker(const Worker &) = delete;
    Worker &operator=(const Worker &) = delete;

    // CMatchingThread::run / CSyncThread::run: the solve, timed, then update_result()
    void run()
    {
        auto t0 = std::chrono::steady_clock::now();
        solve();
        run_time = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
        update_result();
    }
    void start() { thread_ = std::thread([this] { try { run(); } catch (...) { error_ = std::current_exception(); } }); }
    void wait()
    {
        join();
        if (error_) { auto e = error_; error_ = nullptr; std::rethrow_exception(e); }
    }

    volatile int runflag; // the reference's `bool runflag`, written by the UI thread
    float run_time = 0.0f;

protected:
    // joins the worker; a stored exception is dropped (a destructor must not throw: wait() shows it).
    // By now the derived object is gone: a derived class whose solve() / update_result() use its own
    // members calls join() in its destructor, so that the worker never outlives them.
    ~Worker() { join(); }
    void join()
    {
        if (thread_.joinable()) thread_.join();
    }
    virtual void solve() = 0;
    virtual void update_result() = 0;

private:
    std::thread thread_;
    std::exception_ptr error_;
};

} // namespace detail
} // namespace vmorph
#endif
