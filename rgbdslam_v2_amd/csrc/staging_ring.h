// staging_ring.h -- the helper thread of a batch pipeline that copies the caller's pageable images into a ring of `depth`
// page-locked buffers ahead of the calling thread.  Item i uses buffer i % depth, so it is staged once item i - depth, the
// buffer's previous user, has been consumed.  The calling thread waits for an item (wait_staged), reads the buffer and says
// when it is done with it (mark_consumed).  Only the standard library: the staging function is the caller's.
#pragma once
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

namespace rgbdfe {

class StagingRing {
 public:
  // stage(i) runs on the helper thread for i = 0 .. n_items - 1 in order; n_items <= 0: no thread
  StagingRing(int n_items, int depth, std::function<void(int)> stage) : n_(n_items), depth_(depth), stage_(std::move(stage)) {
    if (n_ > 0) th_ = std::thread([this] { run(); });
  }
  // whatever happens to the caller (an exception on its way to the ABI barrier included): the helper is told to stop and joined
  ~StagingRing() { stop(); }
  StagingRing(const StagingRing&) = delete;
  StagingRing& operator=(const StagingRing&) = delete;

  void wait_staged(int i) {
    std::unique_lock<std::mutex> l(m_);
    cv_.wait(l, [&] { return staged_ > i; });
  }
  void mark_consumed(int i) {
    { std::lock_guard<std::mutex> l(m_); consumed_ = i + 1; }
    cv_.notify_all();
  }
  // returns once the helper has left: an item it is staging is finished, none is begun
  void stop() {
    { std::lock_guard<std::mutex> l(m_); stop_ = true; }
    cv_.notify_all();
    if (th_.joinable()) th_.join();
  }

 private:
  void run() {
    for (int i = 0; i < n_; ++i) {
      {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return stop_ || consumed_ >= i - depth_ + 1; });
        if (stop_) return;
      }
      stage_(i);
      { std::lock_guard<std::mutex> l(m_); staged_ = i + 1; }
      cv_.notify_all();
    }
  }
  const int n_, depth_;
  const std::function<void(int)> stage_;
  std::mutex m_;
  std::condition_variable cv_;
  int staged_ = 0, consumed_ = 0;  // items staged by the helper / consumed by the caller
  bool stop_ = false;
  std::thread th_;  // last: it starts in the constructor and reads everything above
};

}  // namespace rgbdfe
