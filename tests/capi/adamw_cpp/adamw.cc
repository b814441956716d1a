// AdamW through the C++ wrapper and the typed C entry points: a small MLP trains with
// flexflow::AdamWOptimizer, then a second optimizer made by the C functions replaces it.
//   ./adamw -b 4 --iterations 2
#include "common.hpp"

using namespace ffx;

int main(int argc, char** argv) {
  Args args(argc, argv);
  FFConfig cfg(argc, argv);
  FFModel ff(cfg);
  const int b = cfg.batch_size();
  Tensor x = ff.create_tensor({b, 24});
  Tensor t = ff.dense(x, 33, AC_MODE_RELU, true);
  t = ff.softmax(ff.dense(t, 10, AC_MODE_NONE, true));
  AdamWOptimizer opt(ff, 0.01, 0.9, 0.999, 0.01, 1e-8, true);
  ff.compile(opt, LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, {METRICS_ACCURACY});
  opt.set_learning_rate(0.005);
  std::mt19937 rng(0);
  feed_normal(ff, x, rng);
  feed_labels(ff, true, 10, rng);
  train_loop(ff, "adamw", args);
  // the C entry points
  flexflow_adamw_optimizer_t h = flexflow_adamw_optimizer_create(ff.raw(), 0.002, 0.9, 0.99, 0.1, 1e-8, false);
  if (!h.impl) {
    std::printf("flexflow_adamw_optimizer_create failed: %s\n", flexflow_last_error());
    return 1;
  }
  flexflow_adamw_optimizer_set_lr(h, 0.001);
  flexflow_model_set_adamw_optimizer(ff.raw(), h);
  ff.train_step();
  std::printf("adamw: C handle step ok, loss %.5f\n", ff.loss());
  flexflow_adamw_optimizer_destroy(h);
  return 0;
}
