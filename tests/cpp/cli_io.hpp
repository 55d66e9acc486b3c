// cli_io.hpp -- what the request-file drivers of tests/cpp share: reading a binary request (a short read ends the
// program with status 2), device buffers whose bytes start as 0xF9 (rows a call leaves alone keep them), and writing
// the response.  Host vectors are allocated one element larger than they are long, so that data() is never null for an
// empty array.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/okvfe.h"

template <typename T>
static void rd(FILE* f, T* p, size_t n) {
  if (n && fread(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
}
template <typename T>
static std::vector<T> rdv(FILE* f, size_t n) {
  std::vector<T> v(n + 1);
  rd(f, v.data(), n);
  v.resize(n);
  return v;
}

template <typename T>
static std::vector<T> download(const void* d, size_t n) {  // n elements of device memory, the default stream drained
  std::vector<T> v(n + 1);
  if (n && okvfe_copy_to_host(v.data(), d, n * sizeof(T), nullptr) != OKVFE_OK) exit(6);
  if (okvfe_stream_synchronize(nullptr) != OKVFE_OK) exit(6);
  v.resize(n);
  return v;
}
template <typename T>
static void put(FILE* o, const std::vector<T>& v) {
  fwrite(v.data(), sizeof(T), v.size(), o);
}

struct DeviceBuffer {
  void* d = nullptr;
  size_t bytes;
  explicit DeviceBuffer(size_t n) : bytes(n ? n : 1) {
    if (okvfe_device_alloc(0, bytes, &d) != OKVFE_OK || okvfe_device_fill(d, 0xF9, bytes, nullptr) != OKVFE_OK) exit(5);
  }
  DeviceBuffer(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { okvfe_device_free(d); }
  template <typename T>
  T* as() const { return static_cast<T*>(d); }
  void upload(const void* src, size_t n) const {
    if (n && okvfe_copy_to_device(d, src, n, nullptr) != OKVFE_OK) exit(5);
  }
  template <typename T>
  void upload(const std::vector<T>& v) const { upload(v.data(), v.size() * sizeof(T)); }
  template <typename T>
  std::vector<T> download(size_t n) const { return ::download<T>(d, n); }
};
