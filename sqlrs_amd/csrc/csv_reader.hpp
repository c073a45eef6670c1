// csv_reader.hpp — the CSV reader's state, shared by its host parser (plumbing.hip) and its device parser (csv_device.hip)
#pragma once

#include <fstream>

#include "common.hpp"

namespace sq {
struct CsvDevice;
}

struct sqlrs_csv {
  sq::Ctx *ctx = nullptr;
  std::ifstream file;
  char delimiter = ',';
  int64_t batch_size = 1024;
  std::vector<std::string> names;
  std::vector<int32_t> dtypes;
  std::vector<int> projection; // indices into the file's columns
  uint64_t remaining = ~0ull;  // records still allowed by the bounds
  uint64_t line = 0;           // for error messages
  bool has_header = true;
  bool started = false;        // sqlrs_csv_next_batch has been called
  std::shared_ptr<sq::CsvDevice> dev; // sqlrs_csv_set_device_parse: the device parser's state (null: host parser)
  bool device_quotes = false;  // sqlrs_csv_set_device_quotes: the device parser also takes pieces whose quotes are all regular
};

namespace sq {
// next batch of <= batch_size records from r->file's position, parsed on the host; *out = NULL at the end (plumbing.hip)
void csv_host_next_batch(sqlrs_csv *r, int out_mem, sqlrs_batch_t **out);
// the same stream of batches, the bytes -> columns work done by the kernels of csv_kernels.hpp (csv_device.hip)
void csv_device_next_batch(sqlrs_csv *r, int out_mem, sqlrs_batch_t **out);
} // namespace sq
