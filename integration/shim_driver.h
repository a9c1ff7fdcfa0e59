// The skeleton every CI driver of the map point store shares: the command line, the context, the output file and the exit codes.
//   usage: <driver> <input.txt> .. (n_inputs of them) <output.txt> [device [driver's own arguments ..]]
// Exit codes, the same for every driver:
//   0  done, the output is complete
//   1  a step failed: the driver named it on stderr, with dsh_last_error
//   2  usage, an input that cannot be read or is malformed, or an output that cannot be opened
//   3  dsh_create failed
// The body runs between dsh_create and dsh_destroy and owns its stores, so they are gone before the context is.  It returns one of the
// codes above; driver_fail and driver_bad_input print the message and give the code.
#pragma once
#include <cstdio>
#include <cstdlib>

#include "../include/defslam_hip.h"

struct DriverArgs {
  dsh_ctx* ctx;
  char** in;          // the n_inputs input paths
  std::FILE* out;
  int n_extra;        // the arguments behind the device
  char** extra;
};

inline int driver_fail(dsh_ctx* ctx, const char* what) {
  std::fprintf(stderr, "%s: %s\n", what, dsh_last_error(ctx));
  return 1;
}

inline int driver_bad_input(const char* path) {
  std::fprintf(stderr, "cannot read %s\n", path);
  return 2;
}

template <class Body>
int run_driver(int argc, char** argv, int n_inputs, Body body) {
  if (argc < n_inputs + 2) {
    std::fprintf(stderr, "usage: %s <input.txt> x %d <output.txt> [device ..]\n", argv[0], n_inputs);
    return 2;
  }
  const int a_out = n_inputs + 1, a_dev = n_inputs + 2, n_extra = argc > a_dev + 1 ? argc - a_dev - 1 : 0;
  std::FILE* out = std::fopen(argv[a_out], "w");
  if (!out) {
    std::fprintf(stderr, "cannot write %s\n", argv[a_out]);
    return 2;
  }
  dsh_ctx* ctx = nullptr;
  int rc = 3;
  if (dsh_create(&ctx, argc > a_dev ? std::atoi(argv[a_dev]) : 0) != DSH_OK) {
    std::fprintf(stderr, "dsh_create failed\n");
  } else {
    DriverArgs a = {ctx, argv + 1, out, n_extra, n_extra ? argv + a_dev + 1 : nullptr};
    rc = body(a);
    dsh_destroy(ctx);
  }
  std::fclose(out);
  return rc;
}
