// Stand-in for ndarray's <ndarray/ndarray_group_stream.hh>: declarations only, of what the YAML / netCDF
// ingest path names.  Nothing here is ever called: the driver fills the grid and solution objects directly.
#pragma once
#include <cstddef>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace ftk {

struct ndarray_base {
    virtual ~ndarray_base() = default;
    virtual int type() const { return 0; }
    static std::string dtype2str(int) { return "unknown"; }
};

template <typename T>
struct ndarray : ndarray_base {
    const std::vector<T>& std_vector() const { return data; }
    std::vector<T> data;
};

struct ndarray_group {
    bool has(const std::string& key) const { return arrays.count(key) != 0; }
    std::shared_ptr<ndarray_base> get(const std::string& key) const { return arrays.at(key); }
    std::map<std::string, std::shared_ptr<ndarray_base>> arrays;
};

struct substream {
    std::vector<std::string> filenames;
};

struct stream {
    std::vector<std::shared_ptr<substream>> substreams;
    std::string path_prefix;
    void parse_yaml(const std::string&) {}
    std::shared_ptr<ndarray_group> read_static() { return std::make_shared<ndarray_group>(); }
    std::shared_ptr<ndarray_group> read(int) { return std::make_shared<ndarray_group>(); }
};

} // namespace ftk
